"""tests/head_ref.py on the CPU: the per-sample float64 reference of the actor loss heads against
float64 autograd through the project's dense path, the conditions on the cases that
tests/test_gpu_actor_heads.py runs on, and the yardstick its tolerances come from (the same dense
functions in f32), so that a miss on the GPU is the kernels'."""
import json
import math

import pytest
import torch

from tests import head_ref as H

A = H.A
CASES = H.cases()
IDS = [f"{T}x{n}-{'stats' if st else 'raw'}" for T, n, st in CASES]


def test_log_prob_is_categorical_log_prob():
    """head_ref.log_prob (the dense path's log-probability with the f32 clamp at any dtype) is
    a2c_vec.categorical_log_prob bit for bit on f32 inputs, edge samples included."""
    c = H.case(5, 103, True)
    pm = A.masked_probs(c.p64().float(), c.m)
    assert torch.equal(H.log_prob(pm, c.acts), A.categorical_log_prob(pm, c.acts))


@pytest.mark.parametrize("T,n,stats", CASES, ids=IDS)
def test_reference_equals_dense_float64(T, n, stats):
    """The reference's per-sample gradients, log-probabilities, per-sample terms and losses equal
    float64 autograd through masked_probs, categorical_log_prob (clamped at eps32) and entropy_of
    upcast to float64, for every head, on every sample of the case (every edge kind): gradients to
    1e-12 of their magnitude, the rest to 1e-12 relative."""
    c = H.case(T, n, stats)
    for head in H.HEADS:
        ref = H.reference(c, head)
        grad, logp, loss, terms, _ = H.dense(c, head, torch.float64, flags=ref.flags64)
        sel = c.valid().expand_as(grad)
        assert bool(torch.isfinite(ref.grad[sel]).all()) and bool(torch.isfinite(grad[sel]).all()), head
        assert bool(((grad - ref.grad).abs() <= 1e-12 * ref.mag)[sel].all()), head
        assert bool(((logp - ref.logp).abs() <= 1e-12 * ref.logp.abs().clamp_min(1.0)).all()), head
        assert bool(((terms - ref.terms).abs() <= 1e-12 * ref.term_mags).all()), head
        assert bool(((loss - ref.loss).abs() <= 1e-12 * ref.loss.abs()).all()), head
        # the workgroup sums are the terms' sums over 256 samples each
        B = -(-c.S // H.WG)
        assert ref.sums.shape == (8, B, terms.shape[1])
        for b in range(B):
            want = ref.terms[:, :, b * H.WG:(b + 1) * H.WG].sum(-1)
            assert bool(((ref.sums[:, b] - want).abs() <= 1e-12 * ref.sum_mags[:, b]).all())


@pytest.mark.parametrize("T,n,stats", CASES, ids=IDS)
def test_case_conditions_hold(T, n, stats):
    """What the GPU test relies on: every edge kind present for every agent (cases of fewer samples
    than kinds: as many kinds as samples) with sample 0, the last sample, the last sample of the
    last full workgroup and lanes 63 / 64 among them, each in a group of its own; NaN in every
    padding column of pu; each kind's defining property in the float64 reference; the E7 gradients
    finite in f32 and above 1 (the entropy term's are about 1e-3); the undecided share of the ratios within the cap; the f32 restatement's
    clip flags equal to float64's at every decided sample; the five clip cases of
    test_ppo_head_kernel_matches_torch populated."""
    c = H.case(T, n, stats)
    S = c.S
    special = [s for s in dict.fromkeys([0, S - 1, H.WG * (S // H.WG) - 1, 63, 64]) if 0 <= s < S]
    assert c.slots[:len(special)] == special[:len(c.slots)]
    for a, k in enumerate(H.NACT):
        kinds = set(c.kind[a][c.kind[a] >= 0].tolist())
        if S >= len(H.KINDS):
            assert set(range(len(H.KINDS))) <= kinds, a
        else:
            assert len(kinds) == S
        if S >= H.E11_MIN_SAMPLES:
            assert set(range(H.E11_ID0, H.E11_ID0 + len(H.E11))) <= kinds, a
        assert bool((c.kind[a][c.slots] >= 0).all())
        groups = c.inv[a][c.slots]
        assert len(set(groups.tolist())) == len(c.slots)
        assert all(int((c.inv[a] == g).sum()) == 1 for g in groups.tolist())
        assert int(c.inv[a].max()) == c.U[a] - 1 and len(set(c.inv[a].tolist())) == c.U[a]
        assert bool(torch.isnan(c.pu[a, :, c.U[a]:]).all()) and c.umax > c.U[a]
        assert bool(torch.isfinite(c.pu[a, :, :c.U[a]]).all()) and bool((c.pu[a, k:, :c.U[a]] == 0).all())
    ref = H.reference(c, "a2c")
    pol = ((ref.grad - ref.ent_grad).abs() / ref.mag).amax(1)             # [8, S]: the policy term's share of mag
    k = c.kind
    for name, want in (("E1", math.log(1 - H.E32)), ("E3", math.log(H.E32)), ("E5_1", math.log(1 - H.E32)),
                       ("E2", math.log(H.E32)), ("E4", math.log(1 - H.E32)), ("E5_2", math.log(0.5))):
        assert bool((ref.logp[k == H.kind_id(name)] == want).all()), name
    zero = c.is_kind("E1", "E3", "E5_1", "E5_2", "E5_k", "E9")
    assert bool(ref.policy_zero[zero].all()) and float(pol[zero].max() if bool(zero.any()) else 0.0) <= 1e-12
    live = c.is_kind("E2", "E4", "E6", "E7_40", "E7_70", "E7_80", "E7_100", "E10")
    assert not bool(ref.policy_zero[live].any()) and bool((pol[live] > 1e-3).all())
    e6 = c.is_kind("E6")
    if bool(e6.any()):   # the valid action at p = 0: its entropy gradient is -es log(1e-10)
        at0 = (c.p64() == 0) & (c.m > 0) & e6[:, None, :]
        assert int(at0.sum()) == int(e6.sum())
        want = H.ENT_COEF * float(torch.tensor(1.0 / S).float()) * math.log(1e-10)
        assert bool(((ref.ent_grad[at0] - want).abs() <= 1e-12 * abs(want)).all())
    e7 = c.is_kind("E7_40", "E7_70", "E7_80", "E7_100")
    e8 = c.is_kind("E8")
    if stats:
        assert float(c.std[H.ZERO_STD_AGENT]) == 0.0
    e9 = c.is_kind("E9")
    assert bool((H.adv_n64(c)[e9] == 0).all())
    shares = {}
    for head in H.HEADS:
        ref = H.reference(c, head)
        sel = ((e7 | e8)[:, None, :] & c.valid()).expand_as(ref.grad)
        g32 = ref.grad.float()
        assert bool(torch.isfinite(g32[sel]).all()), head
        if bool(e7.any()) and head in ("a2c", "record"):       # (PPO's clip holds some of them)
            assert float(ref.grad.abs().amax(1)[e7].min()) > 1.0
        if head != "ppo":
            continue
        share = float((~ref.decided).double().mean())
        shares[head] = share
        assert share <= H.UNDECIDED_SHARE, share
        _, _, _, _, flags32 = H.dense(c, head, torch.float32)
        assert bool((flags32 == ref.flags64)[ref.decided].all())
        if S >= H.E11_MIN_SAMPLES:
            adv, r = H.head_operands(c, head)[0], ref.r
            five = [(adv > 0) & (r > H.CLIP_HI), (adv < 0) & (r < H.CLIP_LO), (adv > 0) & (r < H.CLIP_LO),
                    (adv < 0) & (r > H.CLIP_HI), (r > H.CLIP_LO) & (r < H.CLIP_HI)]
            assert all(int(f.sum()) > 0 for f in five), [int(f.sum()) for f in five]
            e11 = c.kind >= H.E11_ID0
            assert bool(ref.decided[e11].all()) and bool((adv[e11] != 0).all())
            assert 0 < int(ref.flags64[e11].sum()) < int(e11.sum())
    print("ACTOR_HEADS " + json.dumps(dict(conditions=IDS[CASES.index((T, n, stats))],
                                           undecided_share=shares.get("ppo", 0.0))))


def test_yardstick():
    """C_yard: the largest error over 2^-24 mag of the dense path in f32 on the CPU (under autograd,
    against the reference under its own clip flags) over all stored gradient elements of all cases
    and heads except E8, and the same for the per-workgroup sums.  The GPU test allows the kernels 3 x
    these; the values are recorded in profiles/actor_heads/README.md."""
    cg, cs, rows = H.yardstick()
    for head in H.HEADS:
        print("ACTOR_HEADS " + json.dumps(dict(yardstick=head, grad=max(r["grad"] for r in rows if r["head"] == head),
                                               sums=max(r["sums"] for r in rows if r["head"] == head))))
    print("ACTOR_HEADS " + json.dumps(dict(C_yard=cg, C_yard_sums=cs)))
    assert math.isfinite(cg) and math.isfinite(cs) and cg > 0 and cs > 0
    # an f32 restatement worse than 2^-12 relative would make the rule 3 x C_yard empty
    assert cg < 2 ** 12 and cs < 2 ** 12
