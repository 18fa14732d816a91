"""The attention kernels (attn_fwd, attn_delta, attn_bwd_dkv, attn_bwd_dq and
the GEMM fallback's attn_p_from_lse / attn_ds) against the fp64 reference and
the bounds of tests/attention_cases.py, on exact permutation inputs, under
running-max stress, and on strided, poisoned and batched layouts."""

import pytest
import torch

import attention_cases as ac

pytestmark = pytest.mark.gpu

GRADS = ("dq", "dk", "dv")


def _hip():
    from novel_view_synthesis_3d_amd.ops import hip_ops
    return hip_ops


def _run(q, k, v, do, kv_swap=False, lse=False):
    """hip_ops.attention forward + backward on (views of) CUDA tensors."""
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    y = _hip().attention(q, k, v, kv_swap)
    y.backward(do)
    out = {"o": y.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}
    if lse:
        out["lse"] = torch.ops.nvs3d.attn_fwd(q.detach(), k.detach(),
                                              v.detach(), kv_swap)[1]
    return out


def _run_case(case, lse=True):
    return _run(case.q.cuda(), case.k.cuda(), case.v.cuda(), case.do.cuda(),
                case.kv_swap, lse)


def _all(checks):
    """Run every check (each prints its figures), then fail on the first."""
    errors = []
    for fn in checks:
        try:
            fn()
        except AssertionError as e:
            errors.append(e)
    if errors:
        raise errors[0]


def _same_bits(a, b, label):
    for n in a:
        assert torch.isfinite(a[n].float()).all(), (label, n)
        assert torch.equal(a[n], b[n]), (label, n)


# ---------------------------------------------------------------------------
# 2. dense parity grid
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kv_swap", [False, True], ids=["self", "swap"])
@pytest.mark.parametrize("gain", ac.GAINS)
@pytest.mark.parametrize("shape", ac.DENSE_SHAPES, ids=str)
def test_dense_parity(shape, gain, kv_swap, monkeypatch):
    B, L, h, d = shape
    case = ac.dense_case(shape, gain, kv_swap)
    label = f"{shape} gain={gain} swap={int(kv_swap)}"
    fused = ac.fused_bwd_eligible(L, d)
    monkeypatch.delenv("NVS3D_ATTN_BWD", raising=False)
    got = _run_case(case)
    checks = [
        lambda: ac.check(got, case, ac.MARGIN_FUSED, "fwd " + label, ("o",)),
        lambda: ac.check_lse(got["lse"], case, "fwd " + label),
        lambda: ac.check(got, case,
                         ac.MARGIN_FUSED if fused else ac.MARGIN_FALLBACK,
                         ("fused " if fused else "fallback ") + label, GRADS),
    ]
    if fused:  # the same input through the GEMM-recompute backward
        monkeypatch.setenv("NVS3D_ATTN_BWD", "gemm")
        gemm = _run_case(case, lse=False)
        assert torch.equal(gemm["o"], got["o"])
        checks.append(lambda: ac.check(gemm, case, ac.MARGIN_FALLBACK,
                                       "fallback " + label, GRADS))
    _all(checks)


# ---------------------------------------------------------------------------
# 3. exact permutation cases
# ---------------------------------------------------------------------------

def _check_perm_grads(got, case, path, label):
    p = case.params
    dq = float(got["dq"].float().abs().max())
    dk = float(got["dk"].float().abs().max())
    dq_max, dk_max = ac.perm_grad_bounds(case, path == "fallback")
    print(f"ATTN perm {path} {label}: max|dq|={dq:.3e} (<= {dq_max:.3e}) "
          f"max|dk|={dk:.3e} (<= {dk_max:.3e}) G={p.G:g}")
    assert dq <= dq_max and dk <= dk_max, (label, path, dq, dk)
    # every path gives the hit the logit G*bf16(scale)*count the forward took
    # its lse from (the fallback scales afterwards only where the scale is a
    # power of two), so exp(0) = 1 exactly
    assert torch.equal(got["dv"].cpu(), case.dv_exp), (label, path)


@pytest.mark.parametrize("kv_swap", [False, True], ids=["self", "swap"])
@pytest.mark.parametrize("shape", ac.PERM_SHAPES, ids=str)
def test_permutation_is_exact(shape, kv_swap, monkeypatch):
    """softmax = a permutation matrix beyond fp32 resolution: o, dv are known
    bitwise; the peak logit (120 to 320) overflows exp unless the max is
    subtracted first."""
    B, L, h, d = shape
    case = ac.perm_case(shape, kv_swap)
    p = case.params
    label = f"{shape} swap={int(kv_swap)}"
    monkeypatch.delenv("NVS3D_ATTN_BWD", raising=False)
    got = _run_case(case)
    assert torch.equal(got["o"].cpu(), case.o_exp), label
    lse_err = float((got["lse"].double().cpu() - p.peak).abs().max())
    print(f"ATTN perm {label}: peak={p.peak:.2f} margin={p.margin:.2f} "
          f"lse_err={lse_err:.3e}")
    assert lse_err <= 1e-3 * p.peak
    fused = ac.fused_bwd_eligible(L, d)
    _check_perm_grads(got, case, "fused" if fused else "fallback", label)
    if fused:
        monkeypatch.setenv("NVS3D_ATTN_BWD", "gemm")
        _check_perm_grads(_run_case(case, lse=False), case, "fallback", label)


@pytest.mark.parametrize("d", [32, 128])
def test_fallback_p_rows_sum_to_one_at_inexact_scale(d):
    """1/sqrt(d) is not a bf16 value for d in {32,128}. There the fallback
    forms its logits from bf16(q*scale) in fp32, as the forward did, so on the
    permutation input P is exactly the permutation matrix. (With bf16 logits
    scaled after the product the hit was exp(peak*1.1e-4) -> 1.0156.)"""
    case = ac.perm_case((2, 128, 3, d), False)
    q, k, v = case.q.cuda(), case.k.cuda(), case.v.cuda()
    _, lse = torch.ops.nvs3d.attn_fwd(q, k, v, False)
    qs = (q.float() * _hip()._ATTN_SCALE[d]).bfloat16().permute(0, 2, 1, 3)
    s = torch.matmul(qs.float(), k.permute(0, 2, 3, 1).float())
    pm = torch.ops.nvs3d.attn_p_from_lse(s.contiguous(), lse, 1.0).float()
    dev = float((pm.sum(-1) - 1).abs().max())
    print(f"ATTN perm d={d}: fallback max|rowsum(P)-1|={dev:.3e}")
    assert dev == 0.0
    assert torch.equal(pm.argmax(-1).cpu(), case.pi)


# ---------------------------------------------------------------------------
# 4. running-max stress
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ac.STRESS_KINDS)
@pytest.mark.parametrize("d", ac.STRESS_DIMS)
def test_running_max_stress(d, kind):
    """Tile maxima rising or falling by ~30 nats per 64-key tile, and all
    logits near -80 or +80: the online-softmax rescale, the -1e30 start of
    the running max, and lsum neither vanishing nor overflowing."""
    case = ac.stress_case(d, kind)
    got = _run_case(case)
    label = f"stress d={d} {kind}"
    for n, t in got.items():
        assert torch.isfinite(t.float()).all(), (label, n)
    _all([lambda: ac.check(got, case, ac.MARGIN_FUSED, label),
          lambda: ac.check_lse(got["lse"], case, label)])


# ---------------------------------------------------------------------------
# 5. layout and isolation (all bitwise)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("L", [64, 128])   # fallback / fused backward
def test_dense_transposed_inputs(L):
    """q, k, v that are (L,B,h,d) tensors transposed to (B,L,h,d): dense and
    non-overlapping, so they pass every stride check, but the output must
    still be laid out as a contiguous (B,L,h,d) array."""
    case = ac.perm_case((2, L, 3, 16), False)
    want = _run_case(case, lse=False)

    def lbhd(t):
        t = t.cuda().transpose(0, 1).contiguous().transpose(0, 1)
        assert t.shape == case.q.shape and not t.is_contiguous()
        assert t.stride() == (3 * 16, 2 * 3 * 16, 16, 1)
        return t

    got = _run(lbhd(case.q), lbhd(case.k), lbhd(case.v), case.do.cuda())
    wrong = int((got["o"] != want["o"]).sum())
    print(f"ATTN dense-transposed L={L}: {wrong} of {want['o'].numel()} "
          "output elements differ from the contiguous call")
    assert got["o"].is_contiguous()
    assert torch.equal(got["o"].cpu(), case.o_exp)
    _same_bits(got, want, f"dense-transposed L={L}")


def _poisoned_views(tensors, widths):
    """Each (B,L,h,d) tensor as a view into a NaN-filled (B,L,width) buffer;
    tensors sharing a width share one buffer, side by side."""
    B, L, h, d = tensors[0].shape
    C = h * d
    bufs, used, views = {}, {}, []
    for t, w in zip(tensors, widths):
        if w not in bufs:
            bufs[w] = torch.full((B, L, w), float("nan"), dtype=t.dtype,
                                 device="cuda")
            used[w] = 0
        view = bufs[w][..., used[w]:used[w] + C].view(B, L, h, d)
        used[w] += C + 8          # an 8-element NaN gap between neighbours
        assert used[w] - 8 <= w
        view.copy_(t)
        assert not view.is_contiguous() and view.stride(1) == w
        views.append(view)
    return views


@pytest.mark.parametrize("layout", ["fused_qkv", "three_buffers"])
@pytest.mark.parametrize("shape", [(2, 128, 3, 16), (2, 64, 3, 32),
                                   (2, 256, 3, 128)], ids=str)
def test_strided_views_in_poisoned_buffers(shape, layout):
    B, L, h, d = shape
    C = h * d
    case = ac.dense_case(shape, 4, True)
    want = _run_case(case, lse=False)
    widths = ([3 * C + 40] * 3 if layout == "fused_qkv"
              else [C + 8, C + 16, C + 24])
    q, k, v = _poisoned_views([case.q, case.k, case.v], widths)
    got = _run(q, k, v, case.do.cuda(), True)
    _same_bits(got, want, f"{layout} {shape}")


@pytest.mark.parametrize("kv_swap", [False, True], ids=["self", "swap"])
@pytest.mark.parametrize("shape", [(4, 128, 3, 32), (4, 64, 3, 256)], ids=str)
def test_batch_pairs_are_isolated(shape, kv_swap):
    """B=4 against each batch pair run alone: any read across the pair
    boundary (or, without kv_swap, across a batch) changes the bits."""
    q, k, v, do = (t.cuda() for t in ac.dense_inputs(shape, 4))
    full = _run(q, k, v, do, kv_swap)
    for b in (0, 2):
        pair = _run(q[b:b + 2], k[b:b + 2], v[b:b + 2], do[b:b + 2], kv_swap)
        _same_bits(pair, {n: t[b:b + 2] for n, t in full.items()},
                   f"pair {b} of {shape}")
    if not kv_swap:
        one = _run(q[1:2], k[1:2], v[1:2], do[1:2])
        _same_bits(one, {n: t[1:2] for n, t in full.items()}, "batch 1")


@pytest.mark.parametrize("shape", [(2, 256, 3, 64), (2, 192, 3, 128)], ids=str)
def test_two_calls_are_bitwise_equal(shape):
    """No atomics anywhere on the path, fused or fallback."""
    case = ac.dense_case(shape, 4, True)
    a, b = _run_case(case), _run_case(case)
    _same_bits(a, b, f"determinism {shape}")


def test_argument_errors():
    def call(shape, kv_swap=False):
        t = torch.zeros(shape, dtype=torch.bfloat16, device="cuda")
        return torch.ops.nvs3d.attn_fwd(t, t, t, kv_swap)

    with pytest.raises(RuntimeError):
        call((2, 96, 3, 16))            # L not a multiple of 64
    with pytest.raises(RuntimeError):
        call((2, 64, 3, 48))            # unsupported head dim
    with pytest.raises(RuntimeError):
        call((3, 64, 3, 16), True)      # kv_swap needs batch pairs
    call((2, 64, 3, 16), True)          # and the valid neighbour launches


# ---------------------------------------------------------------------------
# 6. the three small kernels, directly
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("D", ac.HEAD_DIMS)
def test_attn_delta(D):
    """201 rows: no multiple of the 256/(D/8) rows a block takes, for any D.
    Bound: fp32 rounding of a D-term sum of exact bf16 products."""
    g = torch.Generator().manual_seed(D)
    do = torch.randn(1, 67, 3, D, generator=g).bfloat16()
    o = (torch.randn(1, 67, 3, D, generator=g) + 2.0).bfloat16()
    got = torch.ops.nvs3d.attn_delta(do.cuda(), o.cuda())
    assert got.shape == (1, 67, 3) and got.dtype == torch.float32
    prod = do.double() * o.double()
    err = (got.double().cpu() - prod.sum(-1)).abs()
    bound = D * 2.0 ** -23 * prod.abs().sum(-1)
    worst = float((err / bound).max())
    print(f"ATTN delta D={D}: worst err/bound={worst:.3f}")
    assert (err <= bound).all()


def _sample(numel, n=4096):
    g = torch.Generator().manual_seed(numel)
    idx = torch.randint(0, numel, (n,), generator=g)
    return torch.cat([idx, torch.arange(numel - 8, numel)]).cuda()


# (1,5,2048,2048) is 21.0 M elements: the grid is capped at 8192 blocks x 256
# threads x 8 elements = 16.8 M, so the grid-stride loop takes a second trip
ELT_SHAPES = [(2, 3, 64, 64), (1, 5, 2048, 2048)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=str)
@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("shape", ELT_SHAPES, ids=str)
def test_attn_p_from_lse(shape, scale, dtype):
    """p[b,h,i,j] = exp(s[b,h,i,j]*scale - lse[b,i,h]) to one bf16 rounding:
    at most 2^-8/(1+2^-8) relative, so 2^-8 leaves 1.5e-5 for the fp32
    arithmetic (exp arguments within +-25)."""
    B, H, L, Lk = shape
    torch.manual_seed(L)
    s = (torch.randn(shape, device="cuda") * (3.0 / scale)).to(dtype)
    lse = torch.randn(B, L, H, device="cuda") * 3.0 + 4.0
    p = torch.ops.nvs3d.attn_p_from_lse(s, lse, scale)
    assert p.shape == s.shape and p.dtype == torch.bfloat16
    idx = _sample(s.numel()) if s.numel() > 1 << 20 else \
        torch.arange(s.numel(), device="cuda")
    row = idx // Lk
    b, hh, i = row // (H * L), (row // L) % H, row % L
    want = torch.exp(s.flatten()[idx].double() * scale
                     - lse[b, i, hh].double()).cpu()
    got = p.flatten()[idx].double().cpu()
    rel = float(((got - want).abs() / want).max())
    print(f"ATTN p_from_lse {shape} scale={scale}: worst rel err={rel:.3e}")
    assert float(want.min()) > 1e-30     # no bf16 subnormals in the test
    assert rel <= 2.0 ** -8


@pytest.mark.parametrize("shape", ELT_SHAPES, ids=str)
def test_attn_ds(shape):
    """ds[b,h,i,j] = scale * p[b,h,i,j] * (dp[b,h,i,j] - delta[b,h,i]) to one
    bf16 rounding."""
    B, H, L, Lk = shape
    scale = 0.176776695   # 1/sqrt(32)
    torch.manual_seed(Lk)
    p = torch.rand(shape, device="cuda").bfloat16()
    dp = torch.randn(shape, device="cuda").bfloat16()
    delta = torch.randn(B, H, L, device="cuda")
    ds = torch.ops.nvs3d.attn_ds(p, dp, delta, scale)
    assert ds.shape == p.shape and ds.dtype == torch.bfloat16
    idx = _sample(p.numel()) if p.numel() > 1 << 20 else \
        torch.arange(p.numel(), device="cuda")
    want = (scale * p.flatten()[idx].double()
            * (dp.flatten()[idx].double()
               - delta.flatten()[idx // Lk].double())).cpu()
    got = ds.flatten()[idx].double().cpu()
    err = (got - want).abs()
    rel = float((err / want.abs().clamp_min(1e-30)).max())
    print(f"ATTN ds {shape}: worst rel err={rel:.3e}")
    assert (err <= 2.0 ** -8 * want.abs()).all()
