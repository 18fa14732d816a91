"""CPU checks of tests/attention_cases.py: the generators do what the GPU
tests rely on, and the bf16 models of the kernels' arithmetic stay at or below
two-thirds of the margins the kernels are held to."""

import math

import pytest
import torch

import attention_cases as ac


@pytest.mark.parametrize("kv_swap", [False, True])
def test_ref64_matches_fp64_autograd_of_the_eager_reference(kv_swap):
    """ref64 is an independent einsum formulation; the project's reference
    in float64 (with k/v flipped by swap_frame_pairs) must agree. That
    reference takes its softmax in fp32 whatever the input type, so the
    agreement is to fp32 rounding (values of order 1 to 10), not fp64."""
    q, k, v, do = ac.dense_inputs((2, 64, 3, 16), 4)
    r = ac.ref64(q, k, v, do, kv_swap)
    q2, k2, v2 = (t.double().requires_grad_(True) for t in (q, k, v))
    ks, vs = ((ac.ref.swap_frame_pairs(k2), ac.ref.swap_frame_pairs(v2))
              if kv_swap else (k2, v2))
    o = ac.ref.attention(q2, ks, vs)
    (o * do.double()).sum().backward()
    for got, want in ((r["o"], o), (r["dq"], q2.grad), (r["dk"], k2.grad),
                      (r["dv"], v2.grad)):
        assert float((got - want.detach()).abs().max()) <= 1e-5
    if kv_swap:  # and the swap matters
        assert not torch.allclose(r["o"], ac.ref64(q, k, v, do, False)["o"])


@pytest.mark.parametrize("shape", ac.DENSE_SHAPES, ids=str)
def test_models_stay_below_two_thirds_of_the_margins(shape):
    """The CPU-side proof that a correct kernel can pass, at every shape,
    gain and kv_swap setting of the GPU grid."""
    B, L, h, d = shape
    for gain in ac.GAINS:
        for kv_swap in (False, True):
            case = ac.dense_case(shape, gain, kv_swap)
            label = f"{shape} gain={gain} swap={int(kv_swap)}"
            args = (case.q, case.k, case.v, case.do, kv_swap)
            if ac.fused_bwd_eligible(L, d):
                ac.check(ac.model_fused(*args), case,
                         ac.MODEL_FRACTION * ac.MARGIN_FUSED,
                         "model_fused " + label)
                names = ("dq", "dk", "dv")
            else:
                names = ac.TENSORS
            fb = ac.model_fallback(*args)
            # the forward is the fused kernel on every path
            ac.check(fb, case, ac.MODEL_FRACTION * ac.MARGIN_FUSED,
                     "model_fwd " + label, names=("o",))
            ac.check(fb, case, ac.MODEL_FRACTION * ac.MARGIN_FALLBACK,
                     "model_fallback " + label, names=names[-3:])
            assert case.lse_model_err > 0


@pytest.mark.parametrize("shape", ac.PERM_SHAPES, ids=str)
def test_permutation_inputs_are_exact(shape):
    B, L, h, d = shape
    q, k, v, do, pi, p = ac.perm_inputs(shape)
    assert p.margin >= ac.PERM_MIN_MARGIN and p.c * p.nbits <= d
    assert math.log2(p.G) == int(math.log2(p.G))
    assert L * math.exp(-p.margin) < 2.0 ** -24
    assert math.exp(p.peak) > 3.4e38        # exp without max-subtraction: inf
    # every permutation is one, and they differ across (batch, head)
    assert torch.equal(pi.sort(-1).values,
                       torch.arange(L).expand(B, h, L))
    assert len({tuple(x.tolist()) for x in pi.reshape(-1, L)}) == B * h
    # logits: the hit is at pi(i) with the designed peak and margin
    s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double()) / math.sqrt(d)
    top = s.topk(2, dim=-1)
    assert torch.equal(top.indices[..., 0], pi)
    assert float((top.values[..., 0] - p.peak).abs().max()) < 1e-9
    assert float((top.values[..., 0] - top.values[..., 1]).min()) \
        >= p.margin - 1e-9
    for kv_swap in (False, True):
        case = ac.perm_case(shape, kv_swap)
        assert float((case.ref["o"] - case.o_exp.double()).abs().max()) \
            <= 1e-12
        assert float((case.ref["dv"] - case.dv_exp.double()).abs().max()) \
            <= 1e-12
        assert float((case.ref["lse"] - p.peak).abs().max()) <= 1e-9
        # true dq, dk are far below the 1e-3*G the kernel is held to
        assert float(case.ref["dq"].abs().max()) <= 1e-6 * p.G
        assert float(case.ref["dk"].abs().max()) <= 1e-6 * p.G
        # the fp32/bf16 model of the kernels gives the exact bits
        m = ac.model_fused(case.q, case.k, case.v, case.do, kv_swap)
        assert torch.equal(m["o"], case.o_exp)
        assert torch.equal(m["dv"], case.dv_exp)
        assert float((m["lse"] - p.peak).abs().max()) <= 1e-3 * p.peak
        fb = ac.model_fallback(case.q, case.k, case.v, case.do, kv_swap)
        assert torch.equal(fb["dv"], case.dv_exp)    # for every d
        assert fb["p_dev"] == 0.0
        for got, fallback in ((m, False), (fb, True)):
            dq_max, dk_max = ac.perm_grad_bounds(case, fallback)
            # far below G
            assert dq_max <= 5e-2 * p.G and dk_max <= 5e-2 * p.G
            assert float(got["dq"].float().abs().max()) <= dq_max
            assert float(got["dk"].float().abs().max()) <= dk_max


def test_permutation_swap_expectation_uses_the_other_batch():
    case = ac.perm_case((2, 64, 3, 16), True)
    b, i, hd = 0, 5, 1
    assert torch.equal(case.o_exp[b, i, hd], case.v[1, case.pi[b, hd, i], hd])
    assert torch.equal(case.dv_exp[1, case.pi[b, hd, i], hd],
                       case.do[b, i, hd])


@pytest.mark.parametrize("d", ac.STRESS_DIMS)
@pytest.mark.parametrize("kind", ac.STRESS_KINDS)
def test_stress_logits_are_as_designed(d, kind):
    case = ac.stress_case(d, kind)
    s = torch.einsum("bihd,bjhd->bhij", case.q.double(),
                     case.k.double()) / math.sqrt(d)
    tmax = s.reshape(*s.shape[:3], 4, 64).amax(-1)   # per 64-key tile
    step = tmax[..., 1:] - tmax[..., :-1]
    if kind == "rising":
        assert float(step.min()) >= 25 and float(step.max()) <= 35
    elif kind == "falling":
        assert float(step.max()) <= -25 and float(step.min()) >= -35
    elif kind == "low":
        assert float(s.max()) <= -70 and float(s.min()) >= -90
    else:
        assert float(s.min()) >= 70 and float(s.max()) <= 90
    assert torch.isfinite(case.ref["lse"]).all()
    # the softmax inside the dominant tile is not degenerate
    assert float(torch.softmax(s, -1).amax(-1).mean()) < 0.5
    m = ac.model_fused(case.q, case.k, case.v, case.do)
    ac.check(m, case, ac.MODEL_FRACTION * ac.MARGIN_FUSED,
             f"model_fused stress d={d} {kind}")
    assert torch.isfinite(m["lse"]).all()
