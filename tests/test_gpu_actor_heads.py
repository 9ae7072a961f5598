"""The three actor loss heads (csrc/fjsp_policy.hip: head_core under k_actor_head<false>,
k_actor_head<true> and k_record_head) against the per-sample float64 reference of
tests/head_ref.py, by direct C calls on its cases: the random batch plus the planted edges (the
inclusive clamp at eps32 and 1 - eps32, the uniform fallback, a valid action at probability 0, a
valid mass down to 2^-100 and a denormal one, advantages of 0 and over 0 + 1e-8, ratios next to the
clip bounds) at sample 0, the last sample, the last sample of the last full workgroup and lanes
63 / 64.

  fjsp_a2c_actor_head, fjsp_a2c_actor_head_ppo (logp_old given, and record mode), fjsp_a2c_record_head
      every stored gradient element within C 2^-24 mag + 2^-149 of float64's, every word of every
      workgroup's sums within C_sum 2^-24 of that workgroup's magnitude sum, C = 3 x C_yard and
      C_sum = 3 x the sums' yardstick (head_ref.yardstick: the dense path in f32 on the CPU, never the
      kernel; measured values in profiles/actor_heads/README.md); logp_out within 4 x 2^-24
      max(|logp64|, 1); the clipped flags equal to float64's at every decided sample and the clipped
      count exact; the gradients whose policy term is exactly 0 unchanged, bit for bit, by the sign of
      the advantages.
  _ActorHead.apply + backward  pu.grad (through fjsp_a2c_run_sums) against the reference gradients
      summed per group.

Every output lies in a larger buffer of NaN sentinels between guard words (Guarded, shared with
test_gpu_backward_edges.py); the padding columns of pu are NaN.  Each case prints its figures on a
line starting ACTOR_HEADS before it asserts."""
import json
import math

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from tests import backward_ref as R  # noqa: E402
from tests import head_ref as H  # noqa: E402
from tests.test_gpu_backward_edges import GUARD, Guarded, _bits, _ptr, _stream  # noqa: E402

A = H.A
U32 = H.U32
UNDERFLOW = 2.0 ** -149
LOGP_FACTOR = 4.0             # the issue's bound on logp_out: 4 u max(|logp64|, 1)
CASES = H.cases()
IDS = [f"{T}x{n}-{'stats' if st else 'raw'}" for T, n, st in CASES]


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from tests import gpu_util  # noqa: F401
    cg, cs, _ = H.yardstick()
    return {"nat": A.nat, "C": 3.0 * cg, "C_sum": 3.0 * cs, "dev": {}}


def _report(**kw):
    print("ACTOR_HEADS " + json.dumps(kw, sort_keys=True))


def _take(g):
    """A Guarded output: guards and the rows past `valid` untouched -> its valid rows on the CPU
    (NaN words in them are the caller's to judge: an unwritten word and a NaN result look alike)."""
    assert bool(torch.isnan(g.buf[:GUARD]).all()) and bool(torch.isnan(g.buf[-GUARD:]).all())
    assert bool(torch.isnan(g.view[g.valid:]).all())
    return g.view[:g.valid].cpu()


def _device(M, c):
    key = (c.T, c.n, c.stats)
    if key not in M["dev"]:
        d = {k: getattr(c, k).cuda().contiguous() for k in ("pu", "inv", "masks", "actions", "adv", "logp_old")}
        d["mean"] = None if c.mean is None else c.mean.cuda()
        d["std"] = None if c.std is None else c.std.cuda()
        cnt, wsum, info, count = H.record_operands(c)
        d.update(cnt=cnt.cuda(), wsum=wsum.cuda(), info=info.cuda(), count=count)
        M["dev"][key] = d
    return M["dev"][key]


def run_head(M, c, head, negate=False):
    """One head on a case by direct C calls -> grad f32 [8, 8, S] (rows j >= nact NaN: never stored),
    sums f64 [8, B, K], logp f32 [8, S] or None, after the sentinel checks.  negate: the advantages
    with the other sign (adv and mean negated; the record head's wsum)."""
    nat, L, d = M["nat"], M["nat"].lib(), _device(M, c)
    S, B = c.S, -(-c.S // H.WG)
    V = lambda t: None if t is None else _ptr(t)  # noqa: E731
    grad = torch.full((8, 8, S), float("nan"))
    ic = float(H.head_operands(c, head)[2][0])
    if head == "record":
        sums = torch.empty(8, B, 2, dtype=torch.float64)
        wsum = -d["wsum"] if negate else d["wsum"]
        for a, k in enumerate(H.NACT):
            g, s = Guarded((k + 3, S), k), Guarded((B + 2, 2), B, torch.float64)
            pu_a, inv_a = d["pu"][a].contiguous(), d["inv"][a].contiguous()
            nat.check(L.fjsp_a2c_record_head(V(pu_a), c.umax, V(inv_a), S, k, V(d["info"][a]), V(wsum[a]), V(d["cnt"][a]),
                                             1.0 / float(d["count"][a]), H.ENT_COEF, V(g.view), V(s.view), _stream()))
            torch.cuda.synchronize()
            grad[a, :k], sums[a] = _take(g), _take(s)
        return {"grad": grad, "sums": sums, "logp": None}
    adv, mean = (-d["adv"], None if d["mean"] is None else -d["mean"]) if negate else (d["adv"], d["mean"])
    K = 2 if head == "a2c" else 4
    g, s = Guarded((29 + 3, S), 29), Guarded((8 + 1, B, K), 8, torch.float64)
    lp = Guarded((8 + 1, S), 8) if head != "a2c" else None
    front = (V(d["pu"]), c.umax, V(d["inv"]), c.T, c.n, V(d["masks"]), V(d["actions"]), V(adv), V(mean), V(d["std"]))
    if head == "a2c":
        nat.check(L.fjsp_a2c_actor_head(*front, ic, H.ENT_COEF, V(g.view), V(s.view), _stream()))
    else:
        old = d["logp_old"] if head == "ppo" else None
        nat.check(L.fjsp_a2c_actor_head_ppo(*front, V(old), V(lp.view), H.CLIP_EPS, ic, H.ENT_COEF, V(g.view), V(s.view),
                                            _stream()))
    torch.cuda.synchronize()
    g29 = _take(g)
    for a, k in enumerate(H.NACT):
        grad[a, :k] = g29[H.MASK_OFFS[a]:H.MASK_OFFS[a] + k]
    return {"grad": grad, "sums": _take(s), "logp": None if lp is None else _take(lp)}


def kernel_flags(c, out, ref0, C):
    """The clipped flags of a PPO launch from its outputs: from r = exp(logp_out - logp_old) (the
    kernel's f32 difference, exact to restate) where that is more than 4 u r from the bound, else
    from the stored gradient of the taken action (a clipped sample holds the entropy term alone:
    nearer to it than to half the unclipped policy term, where that half is over twice the gradient's
    tolerance), else float64's."""
    adv = H.head_operands(c, "ppo")[0]
    r = torch.exp((out["logp"] - c.logp_old).double())
    bound = torch.where(adv > 0, torch.full_like(r, H.CLIP_HI), torch.full_like(r, H.CLIP_LO))
    by_r = ((adv > 0) & (r > H.CLIP_HI)) | ((adv < 0) & (r < H.CLIP_LO))
    clear = (r - bound).abs() > 4 * U32 * r
    idx = c.acts[:, None]
    pol = (out["grad"].double() - ref0.ent_grad).gather(1, idx)[:, 0].abs()
    full = (ref0.grad - ref0.ent_grad).gather(1, idx)[:, 0].abs()
    seen = full > 4 * C * U32 * ref0.mag.gather(1, idx)[:, 0]
    by_g = pol < 0.5 * full
    return torch.where(clear, by_r, torch.where(seen, by_g, ref0.flags64)) & (adv != 0)


def check_head(c, head, out, neg, C, C_sum):
    """Every assertion on one head's outputs (out; neg: the same launch with the advantages'
    sign changed, or None); prints the figures first."""
    S = c.S
    valid = c.valid().expand(8, 8, S)
    e8 = c.is_kind("E8")
    grad, sums = out["grad"], out["sums"]
    flags, share, flips = None, 0.0, 0
    if head == "ppo":
        ref0 = H.reference(c, head, torch.zeros(8, S, dtype=torch.bool))
        flags = kernel_flags(c, out, ref0, C)
        share = float((~ref0.decided).double().mean())
        flips = int((flags != ref0.flags64).sum())
    ref = H.reference(c, head, flags)
    finite = bool(torch.isfinite(grad[valid]).all()) and bool(torch.isfinite(sums).all())
    err = (grad.double() - ref.grad).abs()
    bound = C * U32 * ref.mag + UNDERFLOW
    judged = valid & ~e8[:, None, :]
    ratio = torch.where(judged & torch.isfinite(err), err / (U32 * ref.mag).clamp_min(1e-300), torch.zeros_like(err))
    e7 = c.is_kind("E7_40", "E7_70", "E7_80", "E7_100")
    serr = (sums - ref.sums).abs()
    sratio = torch.where(ref.sum_mags > 0, serr / (U32 * ref.sum_mags).clamp_min(1e-300), torch.zeros_like(serr))
    lerr = None
    if out["logp"] is not None:
        lerr = (out["logp"].double() - ref.logp).abs() / (U32 * ref.logp.abs().clamp_min(1.0))
    _report(head=head, T=c.T, n=c.n, stats=c.stats, finite=finite, grad_ratio=float(ratio.max()),
            grad_ratio_e7=float(ratio[e7[:, None, :].expand_as(ratio)].max()) if bool(e7.any()) else 0.0,
            grad_ratio_e8_not_judged=float((err / (U32 * ref.mag).clamp_min(1e-300))[valid & e8[:, None, :]].max())
            if bool(e8.any()) else 0.0,
            nonfinite=int((~torch.isfinite(grad[valid])).sum()), C=C, sums_ratio=float(sratio.max()), C_sum=C_sum,
            logp_ratio=None if lerr is None else float(lerr.max()), undecided_share=share, flags_unlike_float64=flips)
    # written, finite (the NaN padding columns of pu, E7 and E8 included), unstored rows untouched
    assert bool(torch.isnan(grad[~valid]).all())
    assert finite, [(a, s, H.KINDS[int(c.kind[a, s])] if 0 <= int(c.kind[a, s]) < len(H.KINDS) else "-")
                    for a, s in torch.nonzero((~torch.isfinite(grad) & valid).any(1))[:8].tolist()]
    assert bool((err <= bound)[judged].all()), float(ratio.max())
    # the workgroup sums, the partial last workgroup and a workgroup of one sample among them
    assert sums.shape == ref.sums.shape == (8, -(-S // H.WG), 2 if head in ("a2c", "record") else 4)
    assert bool((serr <= C_sum * U32 * ref.sum_mags).all()), float(sratio.max())
    if head in ("ppo", "ppo_record"):
        assert torch.equal(sums[..., 3], H._blocks(ref.clipped.double(), S)), "clipped count"
        assert bool((out["logp"].double() - ref.logp).abs().le(LOGP_FACTOR * U32 * ref.logp.abs().clamp_min(1.0)).all())
        for name, want in (("E1", 1 - H.E32), ("E3", H.E32)):
            got = out["logp"][c.kind == H.kind_id(name)]
            assert torch.equal(_bits(got), _bits(torch.full_like(got, math.log(want)))), name
    if head == "ppo_record":
        assert float(sums[..., 2].abs().max()) == 0.0 and float(sums[..., 3].abs().max()) == 0.0
    if head == "ppo":
        assert bool((flags == ref.flags64)[ref.decided].all())
        assert share <= H.UNDECIDED_SHARE
    # a policy term that is exactly 0 (E1, E3: clamped; E5: the fallback; E9: adv 0) leaves the
    # entropy term alone, whatever the advantage: bit-equal under the other sign.  E2, E4 pass it.
    if neg is not None:
        same = (_bits(grad) == _bits(neg["grad"])).masked_fill(~valid, True).all(1)          # [8, S]
        zero = c.is_kind("E1", "E3", "E5_1", "E5_2", "E5_k", "E9")
        assert bool(ref.policy_zero[zero].all()) and bool(same[ref.policy_zero].all())
        live = c.is_kind("E2", "E4")
        pol = (grad.double() - ref.ent_grad).gather(1, c.acts[:, None])[:, 0].abs()
        full = (ref.grad - ref.ent_grad).gather(1, c.acts[:, None])[:, 0].abs()
        assert not bool(same[live].any()) and bool((pol[live] > 0.5 * full[live]).all()) and bool((full[live] > 0).all())


@pytest.mark.parametrize("head", H.HEADS)
@pytest.mark.parametrize("T,n,stats", CASES, ids=IDS)
def test_head_matches_float64(M, T, n, stats, head):
    """One head on one case: see the module's docstring.  The record head runs every agent's records
    with cnt cycling through 1, 2, 1000 and 2^20."""
    c = H.case(T, n, stats)
    out = run_head(M, c, head)
    neg = run_head(M, c, head, negate=True) if head != "ppo" else None
    check_head(c, head, out, neg, M["C"], M["C_sum"])


def test_heads_agree_on_the_edges(M):
    """The three heads are one head_core: on a case with every edge kind the A2C head's gradient
    equals record mode's bit for bit (tests/test_gpu_ppo.py compares them on random batches only)."""
    c = H.case(1, 257, True)
    a, b = run_head(M, c, "a2c"), run_head(M, c, "ppo_record")
    v = c.valid().expand_as(a["grad"])
    assert bool(torch.isfinite(a["grad"][v]).all())
    assert torch.equal(_bits(a["grad"][v]), _bits(b["grad"][v]))
    assert torch.equal(_bits(a["sums"][..., 1]), _bits(b["sums"][..., 1]))


def test_actor_head_function_matches_float64(M):
    """_ActorHead.apply + backward on the (3, 70) case with statistics: pu.grad [8, 8, Umax] (the
    per-sample gradients summed per group by fjsp_a2c_run_sums) against the reference gradients
    summed per group in float64, within C 2^-24 x the group's summed mag + one f32 rounding of the
    sum (the E8 groups: finite); padding groups and padded actions get exact zeros; the losses under
    backward_ref.LOSS_RTOL / LOSS_ATOL.
    The E7 samples' gradients of up to 1e29 share their rows with groups whose sums are about 1e-3:
    fjsp_a2c_run_sums sums every run on its own (a segmented scan), so they cost their neighbours
    nothing; as differences of plain f64 prefix sums the same sums were off by 2^-53 of the chunk's
    prefix, 1.46e9 x 2^-24 of the group's mag here (printed: err_over_row_prefix_bound, the error
    over 2^-53 x the row's summed |gradient| + the bound)."""
    c = H.case(3, 70, True)
    d = _device(M, c)
    g = A.RowGroups(d["inv"].clone())
    assert g.U == c.U and torch.equal(g.inv, d["inv"])
    um = g.first.shape[1]
    pu = torch.full((8, 8, um), float("nan"), device="cuda")
    k = min(um, c.umax)                                              # both cover every agent's groups
    pu[:, :, :k] = d["pu"][:, :, :k]
    pu.requires_grad_(True)
    loss = A._ActorHead.apply(pu, g, d["masks"], d["actions"], d["adv"], d["mean"], d["std"], float(c.S), 0.01)
    loss.sum().backward()
    ref = H.reference(c, "a2c")
    idx = c.inv[:, None, :].expand(8, 8, c.S)
    want = torch.zeros(8, 8, um, dtype=torch.float64).scatter_add_(2, idx, ref.grad * c.valid())
    mag = torch.zeros(8, 8, um, dtype=torch.float64).scatter_add_(2, idx, ref.mag * c.valid())
    got = pu.grad.cpu().double()
    err = (got - want).abs()
    bound = M["C"] * U32 * mag + U32 * want.abs() + UNDERFLOW
    # an E8 sample is a group of its own: finite is all that is asked of it (as in the direct calls)
    judged = torch.ones(8, 1, um, dtype=torch.bool)
    for a in range(8):
        judged[a, 0, c.inv[a][c.is_kind("E8")[a]]] = False
    judged = judged.expand_as(err) & (mag > 0)
    ratio = torch.where(judged, err / (U32 * mag).clamp_min(1e-300), torch.zeros_like(err))
    rowsum = (ref.grad * c.valid()).abs().sum(2, keepdim=True)                       # [8, 8, 1]
    _report(head="_ActorHead", T=3, n=70, loss=loss.tolist(), loss64=ref.loss.tolist(), C=M["C"],
            grad_ratio=float(ratio.max()),
            err_over_row_prefix_bound=float((err / (2.0 ** -53 * rowsum + bound))[judged].max()))
    assert bool(torch.isfinite(got).all()) and int((~judged[:, 0] & (mag[:, 0] > 0)).sum()) == 8
    assert bool((got[mag == 0] == 0).all())
    assert torch.allclose(loss.detach().cpu().double(), ref.loss, rtol=R.LOSS_RTOL, atol=R.LOSS_ATOL)
    assert bool((err <= bound)[judged].all()), float(ratio.max())


def test_run_sums_do_not_leak_between_groups(M):
    """fjsp_a2c_run_sums with one value of 1e29 among values of 1e-3, in a row of 7-sample groups
    and in a row of 1 500-sample groups (every run crosses a 1 024-position chunk end, so
    k_run_carry completes them): every group's sum within one f32 rounding of its float64 sum + 1e-12
    of its own summed magnitude (test_run_sums_kernel_equals_float64_group_sums's bound, there on
    same-scale values), the groups after the large value included."""
    S = 5000
    gen = torch.Generator().manual_seed(3)
    keys = torch.stack([torch.arange(S) // 7, torch.arange(S) // 1500])
    G = A.RowGroups(keys.cuda())
    assert G.gsorted is not None and torch.equal(G.inv.cpu(), keys)
    vals = torch.randn(2, S, generator=gen) * 1e-3
    vals[0, 40], vals[1, 1600] = 1e29, -1e29
    got = A.run_sums(vals.cuda(), torch.tensor([0, 1], dtype=torch.int32).cuda(), None, G).cpu().double()
    um = G.first.shape[1]
    want = torch.zeros(2, um, dtype=torch.float64).scatter_add_(1, keys, vals.double())
    mag = torch.zeros(2, um, dtype=torch.float64).scatter_add_(1, keys, vals.double().abs())
    err = (got - want).abs()
    tol = torch.finfo(torch.float32).eps * want.abs() + 1e-12 * mag + 1e-300
    _report(kernel="run_sums", worst_err_over_tol=float((err / tol).max()),
            groups=[int(keys[0].max()) + 1, int(keys[1].max()) + 1])
    assert bool((err <= tol).all())
    assert abs(float(got[0, 5])) > 1e28 and abs(float(got[1, 1])) > 1e28
