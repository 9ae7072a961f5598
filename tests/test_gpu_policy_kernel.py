"""fjsp_a2c_policy / fjsp_a2c_policy_step (csrc/fjsp_policy.hip: k_policy, k_policy_step) against
the float64 reference of tests/policy_ref.py on synthetic operands: the probabilities, values and
argmax (A), the draw action by action (B), the station agents' dedup path around its one / two
column-tile switch (C), the uniform fallback and forced tiles (D) and the launch shapes (E).

b = 2 x (the error of the eager torch f32 policy on the same device and operands against float64)
+ 1e-7 bounds the probabilities; r = 16 b + 1e-6 is the distance from a CDF step inside which a
draw may differ (policy_ref.bound / radius).  Every output of a direct fjsp_a2c_policy call lies in
a larger tensor of sentinels (0xEE bytes, NaN floats) with 256 guard bytes on either side.  Each
case prints its figures (a line starting POLICY_EDGES) before it asserts; the measured ones are in
profiles/policy_edges/README.md."""
import ctypes
import json

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from tests import policy_ref as R  # noqa: E402

A = R.A
N = 1000                      # 15 full tiles and one of 40 envs
GUARD = 256                   # bytes
SHAPES = (1, 31, 32, 33, 63, 64, 65, 96, 129)


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from tests import gpu_util
    return {"nat": gpu_util.native, "V": gpu_util.vec_env, "ctx": {}}


def _report(**kw):
    print("POLICY_EDGES " + json.dumps(kw, sort_keys=True))


# ---------------------------------------------------------------- guarded outputs, the launch
class Guarded:
    """A [shape] output inside a larger tensor of sentinels."""

    def __init__(self, shape, dtype):
        self.u8 = dtype == torch.uint8
        self.g = GUARD // torch.empty(0, dtype=dtype).element_size()
        numel = 1
        for d in shape:
            numel *= d
        self.buf = torch.empty(2 * self.g + numel, dtype=dtype, device="cuda")
        self.buf.fill_(0xEE if self.u8 else float("nan"))
        self.view = self.buf[self.g:self.g + numel].view(*shape)

    def _sentinel(self, t):
        return t == 0xEE if self.u8 else torch.isnan(t)

    def check(self, written=True):
        """The guards untouched; every element inside written (or none)."""
        assert bool(self._sentinel(self.buf[:self.g]).all()) and bool(self._sentinel(self.buf[-self.g:]).all())
        inside = self._sentinel(self.view)
        assert not bool(inside.any()) if written else bool(inside.all())
        return self.view


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _seed_tensor(seed):
    return torch.tensor([A._s64(int(seed))], dtype=torch.int64, device="cuda")


def launch(M, c, seed=0, gid0=0, step=0, det=True, actions=True, values=True, probs=True, masks=None):
    """One fjsp_a2c_policy call on context c's weights and operands -> the outputs asked for, on
    the CPU, after the guard checks; an output left out keeps its sentinels."""
    n = c["n"]
    act, val, pr = Guarded((8, n), torch.uint8), Guarded((n,), torch.float32), Guarded((8, 8, n), torch.float32)
    masks = c["masks_d"] if masks is None else masks
    st = _seed_tensor(seed)
    nat = M["nat"]
    nat.check(nat.lib().fjsp_a2c_policy(
        _ptr(c["feats_d"]), _ptr(masks if actions else None), n, _ptr(c["pw_actor"] if actions else None),
        _ptr(c["pw_critic"] if values else None), _ptr(st if actions else None), int(gid0), int(step), int(bool(det)),
        _ptr(act.view if actions else None), _ptr(val.view if values else None),
        _ptr(pr.view if actions and probs else None), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return {"actions": act.check(actions).cpu().long(), "values": val.check(values).cpu(),
            "probs": pr.check(actions and probs).cpu()}


def context(M, kind, okind, n, opseed=3):
    """Weights of set `kind` packed on the GPU, operands (okind, n), their float64 results, the eager
    f32 path's on the GPU and the bounds; computed once and shared."""
    key = (kind, okind, n, opseed)
    if key in M["ctx"]:
        return M["ctx"][key]
    actors, critic = R.networks(kind, 0)
    feats, masks = R.operands(okind, n, opseed)
    lg, pm, v = R.policy64(actors, critic, feats, masks)
    gap = R.preconditions(lg, masks)
    c = dict(kind=kind, n=n, actors=actors, critic=critic, feats=feats, masks=masks, lg=lg, pm=pm, v=v, gap=gap,
             feats_d=feats.cuda(), masks_d=masks.cuda(), m=A.agent_masks(masks, A.mask_index("cpu")))
    ad, cd = actors.to("cuda"), critic.to("cuda")
    c["pw_actor"], c["pw_critic"] = A.pack_policy_weights(ad, cd)
    pm32, v32 = R.policy32(ad, cd, c["feats_d"], c["masks_d"])
    actors.to("cpu"), critic.to("cpu")
    if kind == "iii":
        c["pm"], c["fb"] = R.fallback_probs(masks)           # from the masks alone
    c["e32"] = float((pm32.cpu().double() - c["pm"]).abs().max())
    c["ev32"] = float((v32.cpu().double() - v).abs().max())
    c["b"] = R.bound(c["e32"])
    c["bv"] = 2.0 * c["ev32"] + 1e-7 * max(1.0, float(v.abs().max()))
    c["r"] = R.radius(c["b"])
    M["ctx"][key] = c
    return c


PAD = torch.arange(8)[None, :, None] >= torch.tensor(A.N_ACTIONS)[:, None, None]       # [8, 8, 1] padded actions


def check_probs(c, out, case):
    """Case A on one deterministic launch with probabilities."""
    ep = float((out["probs"].double() - c["pm"]).abs().max())
    ev = float((out["values"].double() - c["v"]).abs().max())
    clear = R.top2_margin(c["pm"]) > 2 * c["b"]
    share = float((~clear).float().mean())
    wrong = int((out["actions"] != torch.argmax(c["pm"], dim=1))[clear].sum())
    _report(case=case, set=c["kind"], n=c["n"], err_probs=ep, err_probs_f32=c["e32"], ratio=ep / max(c["e32"], 1e-300),
            b=c["b"], err_values=ev, err_values_f32=c["ev32"], bv=c["bv"], near_tie_share=share, greedy_wrong=wrong)
    assert ep <= c["b"], (ep, c["b"])
    assert ev <= c["bv"], (ev, c["bv"])
    assert wrong == 0
    assert share <= R.NEAR_TIE_SHARE
    assert bool((out["probs"][PAD.expand_as(out["probs"])] == 0).all())               # exactly 0, not just small


def check_draws(M, c, case, keys=None, masks=None):
    """Case B: the kernel's draw == draw64 wherever x is farther than r from a CDF step, agent by
    agent; every action returned is valid and has probability."""
    excluded = torch.zeros(8)
    wrong = torch.zeros(8)
    draws = 0
    for seed, step, gid0 in (R.draw_keys(c["n"]) if keys is None else keys):
        act = launch(M, c, seed=seed, gid0=gid0, step=step, det=False, probs=False, masks=masks)["actions"]
        ref, dist = R.draw64(c["pm"], seed, gid0, step)
        far = dist > c["r"]
        assert bool((c["m"].gather(1, act[:, None]) == 1).all()) and bool((c["pm"].gather(1, act[:, None]) > 0).all())
        wrong += ((act != ref) & far).float().sum(dim=1)
        excluded += (~far).float().sum(dim=1)
        draws += c["n"]
    share = float(excluded.sum()) / (8 * draws)
    _report(case=case, set=c["kind"], n=c["n"], draws=8 * draws, r=c["r"], excluded_share=share,
            excluded_by_agent=(excluded / draws).tolist(), wrong_by_agent=wrong.tolist())
    assert wrong.tolist() == [0.0] * 8                    # each agent on its own: the AGV's eight actions too
    assert share <= R.DRAW_EXCLUDED_SHARE


# ---------------------------------------------------------------- A, B
@pytest.mark.parametrize("kind", ["i", "ii"])
def test_probabilities_values_and_argmax_against_float64(M, kind):
    c = context(M, kind, "mixed", N)
    check_probs(c, launch(M, c), "A")


@pytest.mark.parametrize("kind", ["i", "ii"])
def test_draws_equal_the_float64_inverse_cdf(M, kind):
    c = context(M, kind, "mixed", N)
    check_draws(M, c, "B")


# ---------------------------------------------------------------- C
def _set_dedup(M, v):
    M["nat"].check(M["nat"].lib().fjsp_set_option(None, b"policy_dedup", v))


@pytest.mark.parametrize("n", [552, 532])
@pytest.mark.parametrize("kind", ["i", "ii"])
def test_station_dedup_at_its_switch(M, kind, n):
    """Tiles with exactly 1, 2, 7, 31, 32, 33, 63 and 64 distinct station inputs (one column tile up
    to 32, two above), rotated over the station agents, and a partial tile (40 envs with 33 distinct
    inputs, 20 with 5): within b of float64, bit-equal with the dedup off, and bit-equal rows for
    equal inputs and masks within a tile."""
    c = context(M, kind, "dedup", n)
    seed, step, gid0 = R.draw_keys(n)[5]
    runs = {}
    try:
        for v in (1, 0):
            _set_dedup(M, v)
            runs[v] = (launch(M, c), launch(M, c, seed=seed, gid0=gid0, step=step, det=False, probs=False))
    finally:
        _set_dedup(M, 1)
    for v in (1, 0):
        check_probs(c, runs[v][0], f"C dedup={v}")
    for k in ("actions", "values", "probs"):
        assert torch.equal(runs[1][0][k], runs[0][0][k]), k
    assert torch.equal(runs[1][1]["actions"], runs[0][1]["actions"])
    ref, dist = R.draw64(c["pm"], seed, gid0, step)
    assert torch.equal(runs[1][1]["actions"][dist > c["r"]], ref[dist > c["r"]])
    bits = c["feats"].view(torch.int32)
    for v in (1, 0):
        p = runs[v][0]["probs"]
        for a in range(2, 8):
            o, mo = A.OBS_OFFS[a], A.MASK_OFFS[a]
            first = {}
            for e in range(n):
                key = (e // 64, tuple(bits[o:o + 3, e].tolist()), tuple(c["masks"][mo:mo + 3, e].tolist()))
                e0 = first.setdefault(key, e)
                assert torch.equal(p[a, :, e], p[a, :, e0]), (v, a, e, e0)
            assert len(first) > sum(R.tile_distinct(n)[a - 2])      # equal inputs under different masks too


# ---------------------------------------------------------------- D
def _check_fallback(M, c, masks, case):
    """Set (iii) under `masks`: the fallback rows bit-equal to 1.0f / k, the others one-hot on j0;
    greedy the lowest valid index / j0; sampled the uniform draw / j0."""
    exp, fb = R.fallback_probs(masks)
    m = A.agent_masks(masks, A.mask_index("cpu"))
    cc = dict(c, pm=exp, m=m, masks_d=masks.cuda())
    out = launch(M, cc)
    p = out["probs"]
    fbx = fb[:, None, :].expand_as(p)
    _report(case=case, set="iii", n=c["n"], fallback_share=float(fb.float().mean()),
            fallback_bits_differ=int((p != exp.float())[fbx].sum()), err_onehot=float((p.double() - exp)[~fbx].abs().max()))
    assert torch.equal(p[fbx], exp.float()[fbx])                                        # 1.0f / k and 0, bit for bit
    assert float((p.double() - exp)[~fbx].abs().max()) <= c["b"]
    assert bool((p[PAD.expand_as(p)] == 0).all())
    j0 = torch.tensor(R.J0)[:, None].expand_as(fb)
    assert torch.equal(out["actions"], torch.where(fb, torch.argmax(m, dim=1), j0))    # first maximum = lowest valid index
    assert float((out["values"].double() - c["v"]).abs().max()) <= c["bv"]
    for seed, step, gid0 in R.draw_keys(c["n"])[:4]:
        act = launch(M, cc, seed=seed, gid0=gid0, step=step, det=False, probs=False)["actions"]
        ref, dist = R.draw64(exp, seed, gid0, step)
        assert bool((m.gather(1, act[:, None]) == 1).all())
        assert torch.equal(act[~fb], j0[~fb])
        far = fb & (dist > c["r"])
        assert torch.equal(act[far], ref[far])
        assert float((fb & ~far).float().sum()) / float(fb.float().sum()) <= R.DRAW_EXCLUDED_SHARE
    return fb


def test_uniform_fallback_and_first_maximum(M):
    c = context(M, "iii", "mixed", N)
    fb = _check_fallback(M, c, c["masks"], "D")
    assert 0.2 < float(fb.float().mean()) < 0.35 and bool(fb.any(dim=1).all())
    k = c["m"].sum(dim=1)
    assert all(bool((fb & (k == kk)).any()) for kk in (1, 2, 3, 7))      # fallbacks over 1, 2, 3 and 7 valid actions


def test_fallback_with_forced_tiles(M):
    """Whole tiles forced for the pickup station and two station agents, not for the others: the
    skipped tiles and the full path tell the same story."""
    c = context(M, "iii", "mixed", N)
    masks = R.force_tiles(c["masks"], (0, 3, 6), range(0, 16, 2))
    R.preconditions(c["lg"], masks)
    fb = _check_fallback(M, c, masks, "D forced")
    assert bool(fb[3, :64].any()) and not bool(fb[3, :64].all())     # a skipped tile holds both kinds


# (seed, step, global env id, agent, u): keys whose 24-bit uniform is exactly 0 or 0.5, found by a
# scan of a2c_vec.counter_uniform (one in 2^24 draws each); the test checks each before it uses it
EXACT_KEYS = ((1, 0, 1638044, 1, 0.0), (1, 0, 7314922, 0, 0.0), (1, 1, 390126, 6, 0.0), (1, 1, 2949051, 2, 0.0),
              (1, 0, 829384, 2, 0.5), (1, 0, 7672275, 0, 0.5), (1, 0, 12179619, 6, 0.5), (1, 0, 11957715, 7, 0.5),
              (1, 1, 2153859, 3, 0.5), (1, 1, 11383609, 4, 0.5))


def test_draw_at_an_exact_cdf_step(M):
    """x == cdf_k exactly belongs to action k (cdf_k < x is strict), and x == cdf_last (u = 0)
    returns the last action WITH probability, never a masked action behind it.  The fallback set
    with two valid actions makes every quantity a power of two: p = 0.5 each, x = 0.5 or 1, in f32
    and float64 alike, so no radius applies.  The pickup station's valid actions are 0 and 2 (a
    zero-probability action in the middle of the CDF), the AGV's 1 and 4 (three masked behind)."""
    valid = {0: (0, 2), 1: (1, 4)}
    for seed, step, gid, a, u in EXACT_KEYS:
        assert float(A.counter_uniform(seed, torch.tensor([gid]), step, "cpu")[a, 0, 0]) == u
        c = context(M, "iii", "mixed", 3)
        masks = torch.ones_like(c["masks"])
        o, na = A.MASK_OFFS[a], A.N_ACTIONS[a]
        v2 = valid.get(a, tuple(j for j in range(na) if j != R.J0[a]))
        masks[o:o + na, 1] = 0
        masks[[o + v2[0], o + v2[1]], 1] = 1
        R.preconditions(c["lg"], masks)
        exp, fb = R.fallback_probs(masks)
        assert bool(fb[a, 1]) and exp[a, :, 1].tolist().count(0.5) == 2
        ref, dist = R.draw64(exp, seed, gid - 1, step)                         # the env is env 1 of the launch
        assert float(dist[a, 1]) == 0.0 and int(ref[a, 1]) == (v2[0] if u == 0.5 else v2[1])
        gids = torch.arange(gid - 1, gid + 2)
        assert torch.equal(A.sample_categorical(exp.float(), A.counter_uniform(seed, gids, step, "cpu")), ref)
        out = launch(M, dict(c, pm=exp), seed=seed, gid0=gid - 1, step=step, det=False, masks=masks.cuda())
        assert torch.equal(out["probs"][a, :, 1], exp[a, :, 1].float())
        assert int(out["actions"][a, 1]) == int(ref[a, 1]), (a, u, out["actions"][a, 1], ref[a, 1])


# ---------------------------------------------------------------- E
@pytest.mark.parametrize("n", SHAPES)
def test_launch_shapes_against_float64(M, n):
    """Case A at one env and around the critic's 32-env and the actors' 64-env tile edges.  At n = 1
    the bounds are maxima over a single sample of torch's f32 error: the value's (1.16e-6) is the
    one that caught the critic's six-roundings-per-block accumulation (1.19e-6 then, 2.4e-7 with
    mfma6_two; profiles/policy_edges/README.md)."""
    c = context(M, "i", "mixed", n)
    check_probs(c, launch(M, c), "E")


@pytest.mark.parametrize("n", SHAPES)
def test_launch_shapes_draws(M, n):
    check_draws(M, context(M, "i", "mixed", n), "E")


@pytest.mark.parametrize("n", SHAPES)
def test_actors_only_and_critic_only_launches(M, n):
    """actions == NULL (masks, actor_w and seed NULL too) and values == NULL (critic_w NULL) give the
    full launch's bits; the output left out keeps its sentinels (launch's guard checks)."""
    c = context(M, "i", "mixed", n)
    full = launch(M, c)
    critic_only = launch(M, c, actions=False)
    assert torch.equal(critic_only["values"], full["values"])
    actors_only = launch(M, c, values=False)
    assert torch.equal(actors_only["actions"], full["actions"]) and torch.equal(actors_only["probs"], full["probs"])
    seed, step, gid0 = R.draw_keys(n)[2]
    s_full = launch(M, c, seed=seed, gid0=gid0, step=step, det=False)
    s_act = launch(M, c, seed=seed, gid0=gid0, step=step, det=False, values=False)
    assert torch.equal(s_act["actions"], s_full["actions"]) and torch.equal(s_act["probs"], s_full["probs"])
    assert torch.equal(s_full["probs"], full["probs"]) and torch.equal(s_full["values"], full["values"])


@pytest.mark.parametrize("kind", ["i", "ii"])
def test_outputs_do_not_depend_on_the_launch_size(M, kind):
    """An env's value, probabilities and actions depend on its own column (and, for a draw, on its
    global id) alone: the first n envs of the 1000-env operands launched on their own, for every n
    of case E, give the big launch's bits, whatever tile they end in."""
    c = context(M, kind, "mixed", N)
    seed, step, gid0 = R.draw_keys(N)[2]
    big, big_s = launch(M, c), launch(M, c, seed=seed, gid0=gid0, step=step, det=False, probs=False)
    for n in SHAPES:
        cn = dict(c, n=n, feats_d=c["feats_d"][:, :n].contiguous(), masks_d=c["masks_d"][:, :n].contiguous())
        out, out_s = launch(M, cn), launch(M, cn, seed=seed, gid0=gid0, step=step, det=False, probs=False)
        assert torch.equal(out["values"], big["values"][:n]), n
        assert torch.equal(out["probs"], big["probs"][:, :, :n]), n
        assert torch.equal(out["actions"], big["actions"][:, :n]) and torch.equal(out_s["actions"], big_s["actions"][:, :n]), n


SLABS = ("feats", "masks", "actions", "values", "rewards", "term", "trunc", "status")
STEPS = 4


def _learner(M, n, fused):
    env = M["V"].FJSPVecEnv(n)
    L = A.VecMultiAgentA2C(env, batch_size=STEPS, seed=0, use_graph=False)    # init_networks(0): weight set (i)
    L.fused_step = fused
    L.reset(seeds=torch.arange(n) + 7, num_orders=25)
    return L


def _rollout(M, L, ops, det, step_fn):
    """STEPS vector steps on synthetic observations: row t of the feats / masks slabs is overwritten
    before step t.  Returns each step's outputs (the next observation included)."""
    b = L._bufs
    rows = []
    for t in range(STEPS):
        b["feats"][t].copy_(ops[t]["feats_d"])
        b["masks"][t].copy_(ops[t]["masks_d"])
        step_fn(t)
        torch.cuda.synchronize()
        rows.append({k: b[k][t + 1 if k in ("feats", "masks") else t].clone() for k in SLABS})
    assert L.env.faults() == 0
    return rows


def _eager_step(M, L, det):
    b, nat = L._bufs, M["nat"]

    def step(t):                                           # as _collect_eager: the policy kernel, then fjsp_step
        L.policy_fused(b["feats"][t], b["masks"][t], t, det, b["actions"][t], b["values"][t])
        nat.check(nat.lib().fjsp_step(L.env.handle, _ptr(b["actions"][t]), None, 1, ctypes.byref(b["outs"][t])))
    return step


def _misaligned_rollout(M, L, ops, det):
    """The fused launch called directly with every fjsp_out base one element past 16-byte alignment
    (the unstaged store path at n = 64)."""
    n, nat = L.N, M["nat"]
    dt = {"rewards": (torch.float64, 8 * n), "term": (torch.uint8, n), "trunc": (torch.uint8, n), "status": (torch.int32, n),
          "next_masks": (torch.int8, 29 * n), "feats": (torch.float32, 38 * n)}
    b = L._bufs
    rows = []
    for t in range(STEPS):
        b["feats"][t].copy_(ops[t]["feats_d"])
        b["masks"][t].copy_(ops[t]["masks_d"])
        bufs = {k: torch.zeros(1 + cnt, dtype=d, device="cuda")[1:] for k, (d, cnt) in dt.items()}
        o = nat.fjsp_out()
        for k, v in bufs.items():
            assert v.data_ptr() % 16 == v.element_size()
            setattr(o, k, v.data_ptr())
        nat.check(nat.lib().fjsp_a2c_policy_step(
            L.env.handle, _ptr(b["feats"][t]), _ptr(b["masks"][t]), _ptr(L._pw_actor), _ptr(L._pw_critic), _ptr(L._rng),
            0, t, int(det), _ptr(b["actions"][t]), _ptr(b["values"][t]), 1, ctypes.byref(o), 0, n,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        rows.append({"feats": bufs["feats"].view(38, n), "masks": bufs["next_masks"].view(29, n), "actions": b["actions"][t].clone(),
                     "values": b["values"][t].clone(), "rewards": bufs["rewards"].view(8, n), "term": bufs["term"],
                     "trunc": bufs["trunc"], "status": bufs["status"]})
    assert L.env.faults() == 0
    return rows


@pytest.mark.parametrize("n", [1, 33, 64, 65, 96])
def test_policy_step_on_synthetic_operands(M, n):
    """k_policy_step == k_policy + fjsp_step byte for byte on the synthetic operands (whatever the
    synthetic masks allow is stepped: an action the env's real state forbids is the reference's
    invalid action), greedy and sampled, with the pickup / AGV tiles split in halves and whole, and
    its actions are the float64 reference's."""
    nat = M["nat"]
    ops = [context(M, "i", "mixed", n, opseed=10 + t) for t in range(STEPS)]
    for det in (True, False):
        for split in (1, 0):
            nat.check(nat.lib().fjsp_set_option(None, b"policy_split", split))
            try:
                Lf, Le = _learner(M, n, True), _learner(M, n, False)
                fused = _rollout(M, Lf, ops, det, lambda t: Lf.policy_step(t, det))
                assert Lf.env.last_kernel() == "k_policy_step"
                eager = _rollout(M, Le, ops, det, _eager_step(M, Le, det))
                mis = _misaligned_rollout(M, _learner(M, n, True), ops, det) if n == 64 else None
            finally:
                nat.check(nat.lib().fjsp_set_option(None, b"policy_split", 1))
            for t in range(STEPS):
                for k in SLABS:
                    assert torch.equal(fused[t][k], eager[t][k]), (det, split, t, k)
                    if mis is not None:
                        assert torch.equal(mis[t][k].view(torch.uint8), fused[t][k].view(torch.uint8)), (det, split, t, k)
                c, act = ops[t], fused[t]["actions"].cpu().long()
                assert float((fused[t]["values"].cpu().double() - c["v"]).abs().max()) <= c["bv"]
                if det:
                    clear = R.top2_margin(c["pm"]) > 2 * c["b"]
                    assert torch.equal(act[clear], torch.argmax(c["pm"], dim=1)[clear])
                else:
                    ref, dist = R.draw64(c["pm"], Lf._rng_host, 0, t)
                    assert torch.equal(act[dist > c["r"]], ref[dist > c["r"]])
                    assert bool((c["m"].gather(1, act[:, None]) == 1).all())
