"""The four-stage nt P16 GEMM (grids of at most one workgroup per CU: eight computing waves fed by four loader waves) against the
two-stage kernel that serves every larger grid.  Both accumulate every output element in the same order (al.bh, ah.bl, ah.bh per
K-step, K-steps and K segments in order) and share their epilogues, so the results must be equal bit for bit -- no tolerance.

Each product is computed once as the lone launch (M = 10 240, N = 528: 240 tiles) and once more on a grid that the launcher gives to
the two-stage kernel: with the rows doubled (A' = cat(A, A), likewise residual and row-scale source: 480 tiles; row tiles are
independent and the dropout mask hashes the flat element index, which the first half keeps), or as member 0 of a batch of three
identical members (720 tiles).  The per-frame sums of the frame_stats epilogue are added with fp32 atomics in any order: they are held
to the relative bound of tests/test_01_p16_gpu.py::test_frame_stats_from_producers."""
import pytest
import torch

pytestmark = pytest.mark.gpu
M0, N0 = 10240, 528
KS = [528, 1056, 1584, 2112]          # 528 and 1584: K % 32 == 16, the K-tail re-fetch
SHAPES = [(M0, k) for k in KS] + [(10000, 528), (9999, 2112)]   # + row tiles that overhang M (the DMA's row clamp), with and without a K tail


@pytest.fixture(scope="module")
def ops():
    import vptr_amd.ops as ops
    return ops


def rnd(dev, shape, seed, scale=1.0):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn(shape, device=dev, generator=g) * scale


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def dbl(t):
    return torch.cat((t, t))


def grids(dev, M, N=N0):
    """(tiles of the single launch, compute units): the launcher picks the four-stage kernel iff tiles <= compute units"""
    return ((M + 127) // 128) * ((N + 175) // 176), torch.cuda.get_device_properties(dev).multi_processor_count


def check_grids(dev, M):
    tiles, cus = grids(dev, M)
    # 2 * tiles - 3 <= the tiles of the doubled rows
    assert tiles <= cus < 2 * tiles - 3, "%d tiles must be a lone grid and %d must not be (%d compute units)" % (tiles, 2 * tiles - 3, cus)


def gemm(ops, A, W, M, K, **kw):
    D = torch.zeros((M, N0), device=A.device)
    ops.gemm_raw(A, W, D, M, N0, K, ops.A_P16, ops.B_P16, **kw)
    return D


def operands(ops, dev, M, K, seed):
    A = ops.to_p16(rnd(dev, (M, K), seed))
    W = ops.to_p16(rnd(dev, (N0, K), seed + 1, K ** -0.5))
    return A, W, rnd(dev, (N0,), seed + 2), rnd(dev, (M, N0), seed + 3)


@pytest.mark.parametrize("M,K", SHAPES)
@pytest.mark.parametrize("p16_out", [False, True], ids=["f32", "p16"])
def test_lone_plain_epilogue(ops, dev, M, K, p16_out):
    """EPI 1: bias, alpha, residual, fp32 or P16 output"""
    check_grids(dev, M)
    A, W, b, r = operands(ops, dev, M, K, 10)
    # bias / alpha: doubled rows and the batch of three identical members
    lone = gemm(ops, A, W, M, K, bias=b, alpha=0.5, d_p16=p16_out)
    two = gemm(ops, dbl(A), W, 2 * M, K, bias=b, alpha=0.5, d_p16=p16_out)
    assert same_bits(lone, two[:M])
    ys = [torch.zeros((M, N0), device=dev) for _ in range(3)]
    ops.gemm_raw(A, W, ys[0], M, N0, K, ops.A_P16, ops.B_P16, bias=b, alpha=0.5, d_p16=p16_out,
                 batch_extra=[(A, W, ys[1], b, 0.5), (A, W, ys[2], b, 0.5)])
    assert same_bits(lone, ys[0]) and same_bits(lone, ys[1]) and same_bits(lone, ys[2])
    # + residual
    lone = gemm(ops, A, W, M, K, bias=b, alpha=0.5, residual=r, d_p16=p16_out)
    two = gemm(ops, dbl(A), W, 2 * M, K, bias=b, alpha=0.5, residual=dbl(r), d_p16=p16_out)
    assert same_bits(lone, two[:M])


@pytest.mark.parametrize("M,K", SHAPES)
def test_lone_rowscale_dropout_epilogue(ops, dev, M, K):
    """EPI 3: row scale + dropout (+ bias, residual): out-projections and linear2"""
    check_grids(dev, M)
    A, W, b, r = operands(ops, dev, M, K, 20)
    seed = torch.full((1,), 0x1234567, dtype=torch.int64, device=dev)
    nrs = (M + 63) // 64
    rs = rnd(dev, (nrs,), 24).abs() + 0.5
    kw = dict(bias=b, rs_div=64, dropout_p=0.1, site=7, seed=seed)
    lone = gemm(ops, A, W, M, K, rowscale=rs, rs_mod=nrs, residual=r, **kw)
    two = gemm(ops, dbl(A), W, 2 * M, K, rowscale=dbl(rs), rs_mod=2 * nrs, residual=dbl(r), **kw)
    assert same_bits(lone, two[:M])
    assert 0.05 < float((lone == r).float().mean()) < 0.15   # the mask is there: a dropped element is its residual
    # dropout alone
    lone = gemm(ops, A, W, M, K, residual=r, **kw)
    two = gemm(ops, dbl(A), W, 2 * M, K, residual=dbl(r), **kw)
    assert same_bits(lone, two[:M])


@pytest.mark.parametrize("M,K", SHAPES)
@pytest.mark.parametrize("p16_out", [False, True], ids=["f32", "p16"])
def test_lone_activation_epilogue(ops, dev, M, K, p16_out):
    """EPI 4: GELU + saved pre-activation + dropout (linear1 of the MLP blocks)"""
    check_grids(dev, M)
    A, W, b, _ = operands(ops, dev, M, K, 30)
    seed = torch.full((1,), 0x7654321, dtype=torch.int64, device=dev)
    pre1, pre2 = torch.zeros((M, N0), device=dev), torch.zeros((2 * M, N0), device=dev)
    kw = dict(bias=b, act=ops.ACT_GELU, dropout_p=0.1, site=3, seed=seed, d_p16=p16_out)
    lone = gemm(ops, A, W, M, K, Dpre=pre1, **kw)
    two = gemm(ops, dbl(A), W, 2 * M, K, Dpre=pre2, **kw)
    assert same_bits(lone, two[:M]) and same_bits(pre1, pre2[:M])
    assert float(pre1.abs().max()) > 0.0


@pytest.mark.parametrize("nseg", [2, 3])
@pytest.mark.parametrize("M,K", [(M0, 528), (M0, 704), (10000, 528)])
def test_lone_k_segments(ops, dev, M, K, nseg):
    """D = sum_s A_s . B_s^T: two and three K segments (K = 528: every segment ends in a tail step), plain and row scale + dropout"""
    check_grids(dev, M)
    As = [ops.to_p16(rnd(dev, (M, K), 40 + s)) for s in range(nseg)]
    Ws = [ops.to_p16(rnd(dev, (N0, K), 50 + s, (nseg * K) ** -0.5)) for s in range(nseg)]
    b, r = rnd(dev, (N0,), 60), rnd(dev, (M, N0), 61)
    seed = torch.full((1,), 0x2468ace, dtype=torch.int64, device=dev)
    nrs = (M + 63) // 64
    rs = rnd(dev, (nrs,), 62).abs() + 0.5
    for kw, kw2 in [(dict(), dict()),
                    (dict(rowscale=rs, rs_mod=nrs, rs_div=64, dropout_p=0.1, site=5, seed=seed),
                     dict(rowscale=dbl(rs), rs_mod=2 * nrs, rs_div=64, dropout_p=0.1, site=5, seed=seed))]:
        lone = gemm(ops, As[0], Ws[0], M, K, bias=b, alpha=0.5, residual=r, kseg_extra=list(zip(As[1:], Ws[1:])), **kw)
        two = gemm(ops, dbl(As[0]), Ws[0], 2 * M, K, bias=b, alpha=0.5, residual=dbl(r),
                   kseg_extra=[(dbl(a), w) for a, w in zip(As[1:], Ws[1:])], **kw2)
        assert same_bits(lone, two[:M])


@pytest.mark.parametrize("K", [528, 2112])
def test_lone_frame_stats(ops, dev, K):
    """the frame_stats epilogue: D bit for bit, the per-frame sums (fp32 atomics) at the bound of test_frame_stats_from_producers"""
    check_grids(dev, M0)
    HW, frames = 64, M0 // 64
    A, W, b, r = operands(ops, dev, M0, K, 70)
    st1, st2 = ops.frame_stats_buffer(frames, dev), ops.frame_stats_buffer(2 * frames, dev)
    lone = gemm(ops, A, W, M0, K, bias=b, residual=r, frame_stats=st1, frame_rows=HW)
    two = gemm(ops, dbl(A), W, 2 * M0, K, bias=b, residual=dbl(r), frame_stats=st2, frame_rows=HW)
    assert same_bits(lone, two[:M0])
    yd = lone.double().view(frames, -1)
    for st in (st1, st2[:frames]):
        assert float(((st[:, 1].double() - (yd ** 2).sum(1)).abs() / (yd ** 2).sum(1)).max()) < 1e-6
        assert float((st[:, 0].double() - yd.sum(1)).abs().max()) < 1e-6 * float(yd.abs().sum(1).max())
    assert float(((st1[:, 1] - st2[:frames, 1]).abs() / st2[:frames, 1]).max()) < 1e-6
    assert float((st1[:, 0] - st2[:frames, 0]).abs().max()) < 1e-6 * float(yd.abs().sum(1).max())
