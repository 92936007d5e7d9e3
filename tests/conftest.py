import atexit
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# the finetuner probes the public tensorized bucket (finetuner.py:395-410); tests opt in explicitly
os.environ.setdefault("KCA_TENSORIZED_PROBE", "0")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (run on the GPU box via gpurun)")
    config.addinivalue_line("markers", "slow: long-running CPU test")


# MIOpen appends the find results of convolution shapes it has not seen to its user db, which
# utils/miopen.py points at the committed tuning/miopen (the product of tools/miopen_tune.sh, not of
# test runs). The tests, and the processes they start, read and extend a throw-away copy instead
# (utils/miopen.py leaves an explicit MIOPEN_USER_DB_PATH alone), so nothing is written into the tree.
_TUNED_DB = os.path.join(ROOT, "tuning", "miopen")
if "MIOPEN_USER_DB_PATH" not in os.environ and os.path.isdir(_TUNED_DB):
    _db = tempfile.mkdtemp(prefix="kca_miopen_db_")
    shutil.copytree(_TUNED_DB, _db, dirs_exist_ok=True)
    os.environ["MIOPEN_USER_DB_PATH"] = _db
    atexit.register(lambda pid=os.getpid(): os.getpid() == pid and shutil.rmtree(_db, ignore_errors=True))


def pytest_collection_modifyitems(config, items):
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)
