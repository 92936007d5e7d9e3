"""``kca_wq_gemm`` (csrc/kernels/gemm_wq.hip) through ``ops.wq_gemm.wq_linear``, per element against fp64.

The planted weights, the inputs and the bounds are those of tests/test_w8_gpu.py and
tests/test_mx4_gpu.py (derived there), since the kernel's contracts are the slab kernels':

    no activation:  |y - ref| <= u * |ref| + 2^-20 * sum_k |x v s|
    activation:     |y - ref| <= u * |ref| + 1.13 * 2^-20 * sum_k |x v s| + A

u = 2^-8 (bf16) / 2^-11 (fp16), A the activation allowance described there.

The kernel as built: a workgroup owns 128 rows of M, so M tiles end at 128, 256, ...; 64 rows of N, or
128 once ceil(N / 128) * ceil(M / 128) >= 256 (``test_wq_gemm_wide_tiles``); K in 128-wide chunks.
"""
import pytest
import torch

from kubernetes_cloud_amd.ops import _lib, mx4, w8
from kubernetes_cloud_amd.ops.wq_gemm import wq_linear

from . import test_mx4_gpu as tm
from . import test_w8_gpu as t8

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
MS = [65, 127, 128, 129, 257, 300]  # 128 | 129 and 256 | 257: the M-tile boundaries
NKS = {"fp8": [(16, 16), (272, 512), (1360, 1008)], "mxfp4": [(16, 32), (272, 512), (1360, 992)]}
DTYPES = [torch.bfloat16, torch.float16]


def _case(fmt, dtype, M, N, K, seed):
    """(x, weight, bias, check(y, bias, act, what)) with the planted rows of the format's own test module."""
    if fmt == "fp8":
        q, g = t8._weights(N, K, seed)
        x = (torch.randn(M, K + 24, generator=g, device=dev) * 0.5).to(dtype)[:, :K]
        b = (torch.randn(N, generator=g, device=dev) * 0.1).to(dtype)
        return x, q, b, lambda y, bias, act, what: t8._check(y, x, q, bias, act, what)
    q, g = tm._weights(N, K, seed)
    x = tm._x(M, K, g, dtype)
    b = (torch.randn(N, generator=g, device=dev) * 0.1).to(dtype)

    def check(y, bias, act, what):
        ref, tol = tm._ref(x, q, bias, act)
        assert bool(torch.isfinite(ref).all())
        tm._check(y, ref, tol, what)

    return x, q, b, check


def _run_case(fmt, dtype, M, N, K, monkeypatch, seed):
    x, q, b, check = _case(fmt, dtype, M, N, K, seed)
    assert x.stride(0) == K + 24
    calls = tm._spy(monkeypatch)
    for act in (0, 1, 2):
        for bias in (None, b):
            first = None
            for pad in (24, 13):  # row stride N + 24: 8-byte-aligned rows (packed stores); N + 13: scalar stores
                buf = torch.full((M + 2, 8 + N + pad - 8), 777.0, device=dev, dtype=dtype)
                ref_buf = buf.clone()
                out = buf[1:M + 1, 8:8 + N]
                del calls[:]
                y = wq_linear(x, q, bias, act, out=out)
                assert y.data_ptr() == out.data_ptr()
                assert calls == [("kca_wq_gemm", 0)], calls  # ONE launch of the tiled kernel
                what = f"wq {fmt} {dtype} M={M} N={N} K={K} act={act} bias={bias is not None} ldy=N+{pad}"
                if first is None:  # both store forms write the same bits: one fp64 reference serves both
                    check(y, bias, act, what)
                    first = y.clone()
                else:
                    assert torch.equal(y, first), what
                # guard rows and columns of the sentinel buffer untouched
                keep = torch.ones_like(buf, dtype=torch.bool)
                keep[1:M + 1, 8:8 + N] = False
                assert torch.equal(buf[keep], ref_buf[keep]), what
                # planted row 0: an all-zero weight row gives exactly 0, or the bias where nothing else rounds
                if bias is None or act == 0:
                    z0 = torch.zeros(M, device=dev, dtype=dtype) if bias is None else bias[0].expand(M)
                    assert torch.equal(y[:, 0], z0), what
                # the same call gives the same bits, with and without `out`
                del calls[:]
                y2 = wq_linear(x, q, bias, act)
                assert calls == [("kca_wq_gemm", 0)], calls
                assert torch.equal(y2, y), what
                assert torch.equal(wq_linear(x, q, bias, act, out=torch.empty_like(y2)), y), what


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("fmt,N,K", [(f, n, k) for f, nks in NKS.items() for n, k in nks])
@pytest.mark.parametrize("dtype", DTYPES)
def test_wq_gemm_per_element(dtype, fmt, N, K, M, monkeypatch):
    """The smallest legal shape (one partly filled workgroup, one K chunk of a single MFMA step's worth);
    N off every tile (272 = 4 * 64 + 16, 1360 = 21 * 64 + 16); K off the 128-wide chunk (1008 = 7 * 128 +
    112, 992 = 7 * 128 + 96); M one past a slab, around both M-tile boundaries and inside a third tile;
    every activation, with and without bias, both store forms. For MXFP4 in fp16 the planted row 3
    (scale bytes 127 + 14 and 127 - 30 alternating) passes only with the block scale applied in fp32."""
    _run_case(fmt, dtype, M, N, K, monkeypatch, seed=M * 131 + N + K)


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_wq_gemm_rows_past_n(dtype, fmt, monkeypatch):
    """N = 37: lanes own rows past N (read from a valid row, never stored) and a lane's four output rows
    straddle N (the packed store's scalar tail); the second wave column lies wholly past N."""
    _run_case(fmt, dtype, 129, 37, 96, monkeypatch, seed=3)


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_wq_gemm_deep_k(dtype, fmt, monkeypatch):
    """K = 6208 = 48 * 128 + 64: an odd number of chunks plus half a chunk, through both slots of the
    weight register ring and both LDS stages many times."""
    _run_case(fmt, dtype, 129, 640, 6208, monkeypatch, seed=4)


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_wq_gemm_wide_tiles(dtype, fmt, monkeypatch):
    """The 128-row N tile: taken from 256 workgroups on -- here ceil(4112 / 128) = 33 by ceil(1000 / 128) =
    8 -- with the last N tile holding 16 rows and the last M tile 104. K = 160: a chunk and a quarter."""
    _run_case(fmt, dtype, 1000, 4112, 160, monkeypatch, seed=5)


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
@pytest.mark.parametrize("M", [1, 64])
def test_wq_linear_small_m_delegates(fmt, M, monkeypatch):
    """M <= 64 is the decode kernels' ground: only their entry point is called, one launch."""
    x, q, b, check = _case(fmt, torch.bfloat16, M, 272, 512, seed=M)
    calls = tm._spy(monkeypatch)
    y = wq_linear(x, q, b, 1)
    assert calls == [("kca_w8_gemm" if fmt == "fp8" else "kca_mx4_gemm", 0)], calls
    check(y, b, 1, f"wq {fmt} delegated M={M}")
    assert torch.equal(y, (w8.w8_linear if fmt == "fp8" else mx4.mx4_linear)(x, q, b, 1))


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_wq_gemm_exact_integers(dtype, fmt, monkeypatch):
    """Settles the K permutation of the chunk (weight bytes against activation pieces) and the byte /
    nibble order of the conversions, with the construction of ``test_mx4_gemm_exact_integers``: small
    integers in x (20 nonzeros of +-1, +-2 per row), weights among +-{1, 2, 3, 4, 6} with unit scales, no
    two rows or columns alike. Every partial sum is an integer below 2^8, exact in fp32 and in both 16-bit
    types, so the result equals the reference bit for bit whatever the summation order."""
    M, N, K = 129, 48, 128
    g = torch.Generator().manual_seed(11)
    mags = torch.tensor([1.0, 2.0, 3.0, 4.0, 6.0])
    pick = torch.randint(0, 5, (N, K), generator=g)
    neg = torch.randint(0, 2, (N, K), generator=g).bool()
    wv = torch.where(neg, -mags[pick], mags[pick])
    assert len({tuple(r.tolist()) for r in wv}) == N and len({tuple(c.tolist()) for c in wv.t()}) == K
    if fmt == "fp8":
        q = w8.W8Weight(wv.to(torch.float8_e4m3fn).view(torch.uint8).contiguous().to(dev), torch.ones(N, device=dev))
    else:
        codes = torch.tensor([2, 4, 5, 6, 7], dtype=torch.uint8)[pick] | (neg.to(torch.uint8) << 3)
        q = mx4.MX4Weight((codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous().to(dev),
                          torch.full((N, K // 32), 127, dtype=torch.uint8, device=dev))
    assert torch.equal(q.values(torch.float32).cpu(), wv)
    x = torch.zeros(M, K)
    vals = torch.tensor([-2.0, -1.0, 1.0, 2.0])
    for m in range(M):
        x[m, torch.randperm(K, generator=g)[:20]] = vals[torch.randint(0, 4, (20,), generator=g)]
    assert len({tuple(r.tolist()) for r in x}) == M
    x = x.to(dev, dtype)
    ref = x.double() @ q.values(torch.float64).t()
    assert float(ref.abs().max()) <= 240 and torch.equal(ref.to(dtype).double(), ref)
    calls = tm._spy(monkeypatch)
    y = wq_linear(x, q)
    assert calls == [("kca_wq_gemm", 0)]
    bad = (y.double() != ref).nonzero()
    assert torch.equal(y.double(), ref), (bad[:8].tolist(), y[tuple(bad[0])].item(), ref[tuple(bad[0])].item())
    ref_fn = w8.w8_linear_reference if fmt == "fp8" else mx4.mx4_linear_reference
    assert torch.equal(y, ref_fn(x, q))


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_wq_linear_unsupported_inputs_take_the_reference_path(dtype, fmt, monkeypatch):
    """A pointer off the 16-byte grid, a non-unit column stride and fp32 x: the result is the reference
    path's, bit for bit, with no launch and nothing written around ``out``; the aligned twin takes the
    kernel."""
    g = torch.Generator(device=dev).manual_seed(7)
    M, N, K = 129, 48, 512
    calls = tm._spy(monkeypatch)
    w = torch.randn(N, K, generator=g, device=dev) * K ** -0.5
    q = w8.quantize_weight(w) if fmt == "fp8" else mx4.quantize_weight(w)
    ref_fn = w8.w8_linear_reference if fmt == "fp8" else mx4.mx4_linear_reference

    def run(x, what):
        b = (torch.randn(N, generator=g, device=dev) * 0.1).to(x.dtype)
        buf = torch.full((M + 2, N + 16), 777.0, device=dev, dtype=x.dtype)
        ref_buf = buf.clone()
        del calls[:]
        y = wq_linear(x, q, b, 1, out=buf[1:M + 1, 8:8 + N])
        assert not any(rc == 0 for _, rc in calls), (what, calls)  # no native launch
        assert torch.equal(y, ref_fn(x, q, b, 1)), what
        keep = torch.ones_like(buf, dtype=torch.bool)
        keep[1:M + 1, 8:8 + N] = False
        assert torch.equal(buf[keep], ref_buf[keep]), what

    flat = (torch.randn(M * K + 8, generator=g, device=dev) * 0.5).to(dtype)
    x = flat[4:4 + M * K].view(M, K)
    assert x.data_ptr() % 16 == 8
    run(x, "misaligned x")
    wide = (torch.randn(M, 2 * K, generator=g, device=dev) * 0.5).to(dtype)
    run(wide[:, ::2], "column stride 2")
    run(torch.randn(M, K, generator=g, device=dev) * 0.5, "fp32 x")
    del calls[:]
    wq_linear(wide[:, ::2].contiguous(), q)
    assert calls == [("kca_wq_gemm", 0)]


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_wq_linear_measured_crossover(fmt, monkeypatch):
    """M = 128 on GPT-J's 4096 x 4096 projection, where the slab loop measured faster (``takes_slab_loop``):
    ``wq_linear`` runs its two launches; one row more is the tiled kernel; and the tiled kernel, asked for
    directly, is correct at the shape it was dispatched away from."""
    from kubernetes_cloud_amd.ops.wq_gemm import takes_slab_loop
    N = K = 4096
    assert takes_slab_loop(128, N, K, 0 if fmt == "fp8" else 1) and not takes_slab_loop(129, N, K, 0)
    assert not takes_slab_loop(128, N, 992, 1) and not takes_slab_loop(128, 12288, K, 0)
    x, q, b, check = _case(fmt, torch.bfloat16, 129, N, K, seed=9)
    x128 = x[:128]
    calls = tm._spy(monkeypatch)
    y = wq_linear(x128, q, b, 1)
    assert calls == [("kca_w8_gemm" if fmt == "fp8" else "kca_mx4_gemm", 0)] * 2, calls
    del calls[:]
    y129 = wq_linear(x, q, b, 1)
    assert calls == [("kca_wq_gemm", 0)], calls
    check(y129, b, 1, f"wq {fmt} M=129 at the crossover shape")
    del calls[:]
    yk = wq_linear(x128, q, b, 1, dispatch=False)
    assert calls == [("kca_wq_gemm", 0)], calls
    assert torch.equal(yk, y129[:128])  # the rows just checked: a row's bits do not depend on how many follow it
    err = (y.float() - yk.float()).abs().max().item()
    print(f"{fmt}: slab loop vs tiled kernel, max |diff| {err:.3e}")


def test_kca_wq_gemm_refuses_what_it_does_not_cover():
    """The entry point's own argument checks: a nonzero status and no launch."""
    x = torch.zeros(128, 64, device=dev, dtype=torch.bfloat16)
    wq = torch.zeros(16, 64, device=dev, dtype=torch.uint8)
    sc = torch.ones(16, device=dev)
    y = torch.full((128, 16), 777.0, device=dev, dtype=torch.bfloat16)

    def rc(K=64, ldx=64, ldy=16, act=0, dt=0, fmt=0, M=128, xoff=0):
        return _lib.call_rc("kca_wq_gemm", x.data_ptr() + xoff, ldx, wq.data_ptr(), sc.data_ptr(), None, y.data_ptr(),
                            ldy, M, 16, K, act, dt, fmt, _lib.stream())

    assert rc(K=24) != 0 and rc(K=48, fmt=1) != 0 and rc(K=0) != 0  # K % 16 (fp8), K % 32 (mxfp4)
    assert rc(ldx=60) != 0 and rc(ldx=68) != 0 and rc(ldy=8) != 0 and rc(xoff=8) != 0
    assert rc(act=3) != 0 and rc(dt=2) != 0 and rc(fmt=2) != 0 and rc(M=0) != 0
    torch.cuda.synchronize()
    assert bool((y == 777.0).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert bool((y == 0).all())
