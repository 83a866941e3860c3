"""The fp32 + residual epilogue of the one-tile 256 x 256 kernel behind sm_set_gemm_epilogue (csrc/gemm256.hip), which requests the residual rows ahead of
the passes that write them, against the earlier epilogue (mode 0) on the same inputs.  The same operations in the same order, so every output must be
IDENTICAL (torch.equal), and stay inside the operator bars of test_gpu_gemm256 against an
fp64 product of the same 16-bit operands (fp32 outputs 1e-5, bf16 5e-3, fp16 6e-4).  Through the C ABI (sm_linear) with the tile hint that forces the
256 x 256 kernels; the residual is the output buffer, as the tower calls out-proj and fc2."""
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SM_TILE_256 = 256
OLD, NEW = 0, 1


@pytest.fixture(scope="module")
def nat():
    from streammind_amd import native, _lib
    _lib.load()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    yield native
    native.set_gemm_epilogue(-1)


def rnd(shape, seed, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


def relerr(a, b):
    return ((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-6)).item()


def operands(M, N, K, dt, seed):
    w = rnd((N, K), seed, K ** -0.5).to(dt)
    x = rnd((M, K), seed + 1).to(dt)
    return w, x, rnd((N,), seed + 2, 0.1), rnd((M, N), seed + 3)


# the smallest shapes that reach every path of the residual epilogue: a partial second row tile (rows >= M neither read nor written), one live row
# in the last tile with two column tiles, and the fc2 shape class (K = 4096, exact tiles)
RES_SHAPES = [(300, 256, 64), (257, 512, 1024), (512, 1024, 4096)]


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("use_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("M,N,K", RES_SHAPES)
def test_residual_prefetch_epilogue_is_bit_identical(nat, M, N, K, use_bias, f16):
    dt = torch.float16 if f16 else torch.bfloat16
    w, x, bias, res = operands(M, N, K, dt, 100 + M)
    wp, xg = nat.pack_weight(w.cuda()), x.cuda()
    bg = bias.cuda() if use_bias else None
    got = {}
    for mode in (OLD, NEW):
        nat.set_gemm_epilogue(mode)
        buf = res.cuda().clone()
        y = nat.linear(xg, wp, N, K, bias=bg, residual=buf, out=buf, tile_hint=SM_TILE_256)
        torch.cuda.synchronize()
        got[mode] = y.clone()
    assert torch.equal(got[NEW], got[OLD])
    ref = x.double() @ w.double().t() + (bias.double() if use_bias else 0) + res.double()
    assert relerr(got[NEW], ref) < 1e-5


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
def test_residual_prefetch_leaves_rows_beyond_m_alone(nat, f16):
    """rows of the output buffer behind M carry a sentinel: the prefetch of the last row tile is clamped to row M - 1 and nothing is written there;
    the same call also writes the 16-bit copy of the rows (out16), the epilogue's second store"""
    M, N, K, PAD = 300, 256, 64, 256
    dt = torch.float16 if f16 else torch.bfloat16
    w, x, bias, res = operands(M, N, K, dt, 7)
    wp, xg, bg = nat.pack_weight(w.cuda()), x.cuda(), bias.cuda()
    got = {}
    for mode in (OLD, NEW):
        nat.set_gemm_epilogue(mode)
        buf = torch.full((M + PAD, N), -12345.5, device="cuda")
        buf[:M] = res.cuda()
        c16 = torch.full((M + PAD, N), 7.0, device="cuda", dtype=dt)
        nat.linear(xg, wp, N, K, bias=bg, residual=buf[:M], out=buf[:M], out16=c16[:M], tile_hint=SM_TILE_256)
        torch.cuda.synchronize()
        assert (buf[M:] == -12345.5).all() and (c16[M:] == 7.0).all()
        got[mode] = (buf[:M].clone(), c16[:M].clone())
    assert torch.equal(got[NEW][0], got[OLD][0]) and torch.equal(got[NEW][1], got[OLD][1])
    assert torch.equal(got[NEW][1], got[NEW][0].to(dt))
    ref = x.double() @ w.double().t() + bias.double() + res.double()
    assert relerr(got[NEW][0], ref) < 1e-5


def test_residual_prefetch_with_a_separate_residual(nat):
    """residual and output in different buffers (the residual is left as it was)"""
    M, N, K = 300, 256, 64
    w, x, bias, res = operands(M, N, K, torch.bfloat16, 17)
    wp, xg, rg = nat.pack_weight(w.cuda()), x.cuda(), res.cuda()
    got = {}
    for mode in (OLD, NEW):
        nat.set_gemm_epilogue(mode)
        got[mode] = nat.linear(xg, wp, N, K, bias=bias.cuda(), residual=rg, tile_hint=SM_TILE_256).clone()
        torch.cuda.synchronize()
    assert torch.equal(rg.cpu(), res)
    assert torch.equal(got[NEW], got[OLD])
    assert relerr(got[NEW], x.double() @ w.double().t() + bias.double() + res.double()) < 1e-5


def test_set_gemm_epilogue_rejects_other_values(nat):
    from streammind_amd._lib import StreamMindHipError
    for bad in (-2, 2):
        with pytest.raises(StreamMindHipError):
            nat.set_gemm_epilogue(bad)
    nat.set_gemm_epilogue(-1)
