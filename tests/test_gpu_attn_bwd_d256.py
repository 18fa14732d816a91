"""The fused attention backward at head dim 256 (attn_bwd_dkv256 with
transpose reads, attn_bwd_dq<256>) against the fp64 reference and the fused
bounds of tests/attention_cases.py. Shapes (B, L, 3, 256): L=128 is one key
tile and two q-tiles (both buffer sets once), L=256 two key tiles with the
ring wrapping, L=384 tile counts that are no power of two; h=3 makes the
block-index decomposition non-trivial."""

import pytest
import torch

import attention_cases as ac
from test_gpu_attention import (GRADS, _hip, _poisoned_views, _run_case,
                                _same_bits)

pytestmark = pytest.mark.gpu


def _direct(q, k, v, do, kv_swap):
    """attn_fwd, attn_delta and attn_bwd_fused called as ops."""
    _hip()   # loads the extension
    ops = torch.ops.nvs3d
    o, lse = ops.attn_fwd(q, k, v, kv_swap)
    dq, dk, dv = ops.attn_bwd_fused(q, k, v, do, lse, ops.attn_delta(do, o),
                                    kv_swap)
    return {"dq": dq, "dk": dk, "dv": dv}


def _direct_case(case):
    return _direct(case.q.cuda(), case.k.cuda(), case.v.cuda(),
                   case.do.cuda(), case.kv_swap)


@pytest.mark.parametrize("kv_swap", [False, True], ids=["self", "swap"])
@pytest.mark.parametrize("gain", ac.GAINS)
@pytest.mark.parametrize("L", [128, 256, 384])
def test_direct_call(L, gain, kv_swap):
    case = ac.dense_case((2, L, 3, 256), gain, kv_swap)
    ac.check(_direct_case(case), case, ac.MARGIN_FUSED,
             f"fused d256 L={L} gain={gain} swap={int(kv_swap)}", GRADS)


@pytest.mark.parametrize("kv_swap", [False, True], ids=["self", "swap"])
@pytest.mark.parametrize("L", [128, 256])
def test_through_autograd(L, kv_swap, monkeypatch):
    case = ac.dense_case((2, L, 3, 256), 4, kv_swap)
    label = f"d256 L={L} swap={int(kv_swap)}"
    monkeypatch.delenv("NVS3D_ATTN_BWD", raising=False)
    got = _run_case(case, lse=False)
    ac.check(got, case, ac.MARGIN_FUSED, "autograd " + label, GRADS)
    want = _direct_case(case)
    _same_bits({n: got[n] for n in GRADS}, want, "dispatch " + label)
    monkeypatch.setenv("NVS3D_ATTN_BWD", "gemm")
    ac.check(_run_case(case, lse=False), case, ac.MARGIN_FALLBACK,
             "gemm " + label, GRADS)


@pytest.mark.parametrize("kv_swap", [False, True], ids=["self", "swap"])
@pytest.mark.parametrize("L", [128, 256])
def test_permutation_inputs(L, kv_swap):
    case = ac.perm_case((2, L, 3, 256), kv_swap)
    got = _direct_case(case)
    dq = float(got["dq"].float().abs().max())
    dk = float(got["dk"].float().abs().max())
    dq_max, dk_max = ac.perm_grad_bounds(case, False)
    print(f"ATTN perm d256 L={L} swap={int(kv_swap)}: max|dq|={dq:.3e} "
          f"(<= {dq_max:.3e}) max|dk|={dk:.3e} (<= {dk_max:.3e})")
    assert torch.equal(got["dv"].cpu(), case.dv_exp)
    assert dq <= dq_max and dk <= dk_max


def test_strided_views_in_poisoned_buffer():
    shape = (2, 128, 3, 256)
    case = ac.dense_case(shape, 4, True)
    want = _direct_case(case)
    q, k, v = _poisoned_views([case.q, case.k, case.v],
                              [3 * 3 * 256 + 40] * 3)
    _same_bits(_direct(q, k, v, case.do.cuda(), True), want, "fused_qkv")


@pytest.mark.parametrize("kv_swap", [False, True], ids=["self", "swap"])
def test_batch_pairs_are_isolated(kv_swap):
    q, k, v, do = (t.cuda() for t in ac.dense_inputs((4, 128, 3, 256), 4))
    full = _direct(q, k, v, do, kv_swap)
    for b in (0, 2):
        pair = _direct(q[b:b + 2], k[b:b + 2], v[b:b + 2], do[b:b + 2],
                       kv_swap)
        _same_bits(pair, {n: t[b:b + 2] for n, t in full.items()},
                   f"pair {b}")


def test_two_calls_are_bitwise_equal():
    case = ac.dense_case((2, 256, 3, 256), 4, True)
    _same_bits(_direct_case(case), _direct_case(case), "determinism d256")
