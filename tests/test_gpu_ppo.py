"""The PPO learner on the GPU (ppo_vec over FJSPVecEnv): the HIP loss head
(fjsp_a2c_actor_head_ppo) against torch autograd and against the A2C head, the grouped HIP path
against the dense torch path from a common state, and the learner end to end.  The clipped
objective is an extension (the reference has A2C only); the CPU side is tests/test_ppo_learner.py."""
import copy
import ctypes
import importlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

EPS_CLIP = 0.2
# every ratio at least 1 % away from a clip bound (0.8, 1.2): f32 rounding cannot flip a sample
RATIOS = (0.5, 0.79, 0.9, 1.0, 1.1, 1.21, 1.6)


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from tests import gpu_util
    return {"A": importlib.import_module("multi-agent-rl-for-fjsp_amd.a2c_vec"),
            "PPO": importlib.import_module("multi-agent-rl-for-fjsp_amd.ppo_vec"),
            "V": importlib.import_module("multi-agent-rl-for-fjsp_amd.vec_env"),
            "nat": gpu_util.native}


def _head_inputs(A, T, n, seed):
    """Random inputs of the loss heads for a [T, ., n] batch: a device grouping of random keys,
    per-group probabilities, masks that always contain the taken action, f64 advantages and their
    statistics.  About a tenth of the samples have a single valid action; every seventh group
    puts all its probability on action 0 while its samples' masks exclude action 0 (no valid
    action has probability left: the uniform fallback)."""
    gen = torch.Generator().manual_seed(seed)
    S = T * n
    U = max(3, S // 5)
    keys = torch.randint(0, U, (8, S), generator=gen)
    g = A.RowGroups((keys * 7919 + 11).cuda())
    um = g.first.shape[1]
    logits = torch.randn(8, 8, um, generator=gen)
    for a, k in enumerate(A.N_ACTIONS):
        logits[a, k:] = float("-inf")
    pu = torch.softmax(logits, dim=1)
    onehot = (torch.arange(um) % 7 == 3)
    pu[:, :, onehot] = 0.0
    pu[:, 0, onehot] = 1.0
    inv = g.inv.cpu()
    m = torch.zeros(8, 8, S)
    acts = torch.zeros(8, S, dtype=torch.long)
    for a, k in enumerate(A.N_ACTIONS):
        m[a, :k] = (torch.rand(k, S, generator=gen) < 0.5).float()
        fb = onehot[inv[a]]                                               # the fallback samples
        act = torch.where(fb, 1 + torch.randint(0, k - 1, (S,), generator=gen), torch.randint(0, k, (S,), generator=gen))
        single = torch.rand(S, generator=gen) < 0.1
        m[a, :k, single] = 0.0
        m[a, 0, fb] = 0.0
        m[a].scatter_(0, act[None], 1.0)
        acts[a] = act
    masks = torch.zeros(T, 29, n, dtype=torch.int8)
    for a, k in enumerate(A.N_ACTIONS):
        masks[:, A.MASK_OFFS[a]:A.MASK_OFFS[a] + k, :] = m[a, :k].reshape(k, T, n).permute(1, 0, 2).to(torch.int8)
    actions = acts.reshape(8, T, n).permute(1, 0, 2).to(torch.uint8).contiguous()
    adv = torch.randn(T, 8, n, generator=gen, dtype=torch.float64) * 2
    # any statistics do for the head (operands): a mean off the advantages' keeps the sums from cancelling
    mean = (torch.randn(8, generator=gen) * 0.1 - 0.3).float()
    std = (0.5 + torch.rand(8, generator=gen)).float()
    adv_n = (adv.float().permute(1, 0, 2).reshape(8, S) - mean[:, None]) / (std[:, None] + 1e-8)
    c = lambda t: t.cuda().contiguous()  # noqa: E731
    return {"g": g, "pu": c(pu), "m": c(m), "acts": c(acts), "masks": c(masks), "actions": c(actions), "adv": c(adv),
            "mean": c(mean), "std": c(std), "adv_n": c(adv_n), "S": S, "gen": gen}


def _constructed_logp_old(A, inp):
    """logp_now - log(r*), r* drawn per (agent, sample) from RATIOS."""
    with torch.no_grad():
        p = inp["g"].gather(inp["pu"])
        logp = A.categorical_log_prob(A.masked_probs(p, inp["m"]), inp["acts"])
    rstar = torch.tensor(RATIOS)[torch.randint(0, len(RATIOS), logp.shape, generator=inp["gen"])].cuda()
    return (logp - torch.log(rstar)).contiguous(), logp


@pytest.mark.parametrize("T,n", [(3, 70), (5, 103), (1, 256)])
def test_ppo_head_kernel_matches_torch(M, T, n):
    """fjsp_a2c_actor_head_ppo against the same loss in torch ops differentiated by autograd
    (ppo_vec.ppo_head_terms): one partial workgroup with n no multiple of 64, several workgroups
    with a partial last one, exactly one full workgroup."""
    A, PPO = M["A"], M["PPO"]
    inp = _head_inputs(A, T, n, seed=5 + T)
    S, g, count, coef = inp["S"], inp["g"], float(inp["S"]), 0.01
    logp_old, _ = _constructed_logp_old(A, inp)
    pu = inp["pu"].clone().requires_grad_(True)
    got, stats = PPO._ActorHeadPPO.apply(pu, g, inp["masks"], inp["actions"], inp["adv"], inp["mean"], inp["std"],
                                         logp_old, None, EPS_CLIP, count, coef)
    got.sum().backward()
    g_got = pu.grad.clone()
    pu.grad = None
    surr, ent, kl, clipped, _ = PPO.ppo_head_terms(g.gather(pu), inp["m"], inp["acts"], inp["adv_n"], logp_old, EPS_CLIP)
    want = -surr.double().sum(1) / count - coef * ent.double().sum(1) / count
    want.sum().backward()
    r = torch.exp(_constructed_logp_old(A, inp)[1] - logp_old)
    lo, hi = 1 - EPS_CLIP, 1 + EPS_CLIP
    an = inp["adv_n"]
    cases = [(an > 0) & (r > hi), (an < 0) & (r < lo), (an > 0) & (r < lo), (an < 0) & (r > hi), (r > lo) & (r < hi)]
    assert all(int(c.sum()) > 0 for c in cases)
    print("loss", got.tolist(), want.tolist())
    print("kl", stats[:, 1].tolist(), kl.double().sum(1).tolist(), "clip", stats[:, 2].tolist())
    got_sum, want_sum = got.detach().double().sum().item(), want.detach().sum().item()
    assert abs(got_sum - want_sum) <= 1e-5 * abs(want_sum), (got_sum, want_sum)
    kl_want = kl.detach().double().sum(1)
    assert float(((stats[:, 1] - kl_want).abs() / kl_want.abs()).max()) <= 1e-5
    assert torch.equal(stats[:, 2].long(), clipped.sum(1))
    assert float(((stats[:, 0] - ent.detach().double().sum(1)).abs() / ent.detach().double().sum(1).abs()).max()) <= 1e-5
    valid = torch.zeros(8, 8, 1, dtype=torch.bool, device="cuda")
    for a, k in enumerate(A.N_ACTIONS):
        valid[a, :k] = True
    sel = valid.expand_as(pu.grad)
    # no element is left out: both gradients are finite everywhere (the per-sample comparison
    # against float64, edge by edge, is tests/test_gpu_actor_heads.py's)
    assert bool(torch.isfinite(g_got).all()) and bool(torch.isfinite(pu.grad[sel]).all())
    d = (g_got - pu.grad)[sel]
    print("grad err", float(d.abs().max()), "scale", float(pu.grad[sel].abs().max()))
    assert float(d.abs().max()) <= 1e-4 * float(pu.grad[sel].abs().max())


def _raw_heads(nat, inp, T, n, logp_old, logp_out):
    """Both C entries on the same inputs -> (A2C grad, A2C sums [8, B, 2], PPO grad, PPO sums [8, B, 4])."""
    S = T * n
    V = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    E = lambda *sh, dt: torch.full(sh, float("nan"), dtype=dt, device="cuda")  # noqa: E731
    B = -(-S // 256)
    g0, s0 = E(29, S, dt=torch.float32), E(8, B, 2, dt=torch.float64)
    g1, s1 = E(29, S, dt=torch.float32), E(8, B, 4, dt=torch.float64)
    pu, g = inp["pu"], inp["g"]
    L = nat.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nat.check(L.fjsp_a2c_actor_head(V(pu), pu.shape[2], V(g.inv), T, n, V(inp["masks"]), V(inp["actions"]), V(inp["adv"]),
                                    V(inp["mean"]), V(inp["std"]), 1.0 / S, 0.01, V(g0), V(s0), st))
    nat.check(L.fjsp_a2c_actor_head_ppo(V(pu), pu.shape[2], V(g.inv), T, n, V(inp["masks"]), V(inp["actions"]),
                                        V(inp["adv"]), V(inp["mean"]), V(inp["std"]), V(logp_old), V(logp_out), EPS_CLIP,
                                        1.0 / S, 0.01, V(g1), V(s1), st))
    torch.cuda.synchronize()
    return g0, s0, g1, s1


@pytest.mark.parametrize("T,n", [(3, 70), (5, 103), (1, 256)])
def test_record_mode_equals_a2c_head(M, T, n):
    """logp_old = NULL: the ratio is 1, so the gradient and the entropy sums are fjsp_a2c_actor_head's
    bit for bit, the KL and clip sums exactly 0, and logp_out holds the log-probabilities."""
    A, nat = M["A"], M["nat"]
    inp = _head_inputs(A, T, n, seed=9 + T)
    S = inp["S"]
    logp_out = torch.full((8, S), float("nan"), device="cuda")
    g0, s0, g1, s1 = _raw_heads(nat, inp, T, n, None, logp_out)
    assert not bool(torch.isnan(g1).any()) and not bool(torch.isnan(s1).any())      # every element written
    assert torch.equal(g0, g1)
    assert torch.equal(s0[..., 1], s1[..., 1])
    assert float(s1[..., 2].abs().max()) == 0.0 and float(s1[..., 3].abs().max()) == 0.0
    # sum surr = sum adv_n at ratio 1
    assert torch.allclose(s1[..., 0].sum(1), inp["adv_n"].double().sum(1), rtol=1e-6, atol=1e-6)
    _, logp = _constructed_logp_old(A, inp)
    assert float((logp_out - logp).abs().max()) <= 1e-6


@pytest.mark.parametrize("T,n", [(3, 70), (5, 103)])
def test_record_head_equals_a2c_head(M, T, n):
    """fjsp_a2c_record_head on one record per sample (cnt = 1, wsum = the f32 advantage widened to
    f64, info = mask bits | action << 8) against fjsp_a2c_actor_head on the same f64 values without
    normalisation, agent by agent: both are head_core, so the gradient rows and (1 * entropy being
    exact) the workgroups' entropy sums agree bit for bit.  The A2C head rounds each adv * logp to
    f32 (<= 2^-24 relative) and the record head multiplies in f64, so the workgroups' adv logp sums
    differ by at most 2^-23 sum |adv logp| over the workgroup's samples (the factor 2 covers the
    f64 summation)."""
    A, nat = M["A"], M["nat"]
    inp = _head_inputs(A, T, n, seed=13 + T)
    S, pu, g = inp["S"], inp["pu"], inp["g"]
    B = -(-S // 256)
    adv = inp["adv"].float().double().contiguous()                              # [T, 8, n]
    V = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    E = lambda *sh, dt: torch.full(sh, float("nan"), dtype=dt, device="cuda")  # noqa: E731
    L = nat.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g0, s0, s1 = E(29, S, dt=torch.float32), E(8, B, 2, dt=torch.float64), E(8, B, 4, dt=torch.float64)
    g1, logp = E(29, S, dt=torch.float32), E(8, S, dt=torch.float32)            # logp: the kernels' own
    nat.check(L.fjsp_a2c_actor_head(V(pu), pu.shape[2], V(g.inv), T, n, V(inp["masks"]), V(inp["actions"]), V(adv),
                                    None, None, 1.0 / S, 0.01, V(g0), V(s0), st))
    nat.check(L.fjsp_a2c_actor_head_ppo(V(pu), pu.shape[2], V(g.inv), T, n, V(inp["masks"]), V(inp["actions"]), V(adv),
                                        None, None, None, V(logp), EPS_CLIP, 1.0 / S, 0.01, V(g1), V(s1), st))
    bits = (inp["m"].to(torch.int32) << torch.arange(8, device="cuda", dtype=torch.int32)[None, :, None]).sum(1)
    info = (bits | (inp["acts"].to(torch.int32) << 8)).to(torch.int32).contiguous()    # [8, S]
    wsum = adv.permute(1, 0, 2).reshape(8, S).contiguous()
    cnt = torch.ones(S, dtype=torch.int32, device="cuda")
    terms = torch.nn.functional.pad((wsum * logp.double()).abs(), (0, B * 256 - S)).view(8, B, 256).sum(2)
    for a, k in enumerate(A.N_ACTIONS):
        gr, sr = E(k, S, dt=torch.float32), E(B, 2, dt=torch.float64)
        nat.check(L.fjsp_a2c_record_head(V(pu[a]), pu.shape[2], V(g.inv[a]), S, k, V(info[a]), V(wsum[a]), V(cnt),
                                         1.0 / S, 0.01, V(gr), V(sr), st))
        torch.cuda.synchronize()
        assert not bool(torch.isnan(gr).any()) and not bool(torch.isnan(sr).any())   # every element written
        o = A.MASK_OFFS[a]
        assert torch.equal(g0[o:o + k], gr), a
        assert torch.equal(s0[a, :, 1], sr[:, 1]), a
        d, bound = (s0[a, :, 0] - sr[:, 0]).abs(), 2.0 ** -23 * terms[a]
        print("agent", a, "adv logp sums: diff", d.tolist(), "bound", bound.tolist())
        assert bool((d <= bound).all()), a


def _flat_split(params, flat):
    out, o = [], 0
    for p in params:
        out.append(flat[o:o + p.numel()])
        o += p.numel()
    return out


def test_grouped_hip_epoch_equals_dense_epoch(M):
    """One collected 128-env x 16-step batch: epoch 0 (record mode), then the same state
    (parameters, both Adam states, logp_old) given to two learners that run one further epoch, one
    on the grouped HIP path and one dense in torch ops: the same gradients and losses
    (test_a2c_4096_envs_grouped_update's tolerances).  Few samples clip at the default range here;
    the clipping itself is test_ppo_head_kernel_matches_torch's, with constructed margins."""
    A, PPO, V = M["A"], M["PPO"], M["V"]
    n, T = 128, 16
    learner = PPO.VecMultiAgentPPO(V.FJSPVecEnv(n), batch_size=T, seed=12)
    learner.reset(seeds=torch.arange(n) + 3, num_orders=25)
    learner.collect()
    b = learner._bufs
    ret, adv = learner.advantages()
    args = (b["feats"][:T], b["masks"][:T], b["actions"], ret, adv, learner.gidx, learner.midx)
    bg = PPO.PPOBatch(*args, dedup=True)
    bd = PPO.PPOBatch(*args, dedup=False)
    assert bg.head_kernel and bg.coef is not None and not bd.head_kernel
    hp = (learner.entropy_coef, learner.max_grad_norm, learner.ppo_clip)
    PPO.ppo_epoch(bg, learner.actors, learner.critic, learner.optim_actor, learner.optim_critic, *hp)
    bd.logp_old = bg.logp_old.clone()
    res = []
    for batch in (bd, bg):
        actors, critic = copy.deepcopy(learner.actors), copy.deepcopy(learner.critic)
        oa = torch.optim.Adam(actors.parameters(), lr=3e-4, fused=True, capturable=True)
        oc = torch.optim.Adam(critic.parameters(), lr=1e-3, fused=True, capturable=True)
        oa.load_state_dict(copy.deepcopy(learner.optim_actor.state_dict()))
        oc.load_state_dict(copy.deepcopy(learner.optim_critic.state_dict()))
        probe = []
        al, cl, stats = PPO.ppo_epoch(batch, actors, critic, oa, oc, *hp, grad_probe=probe.append)
        res.append((al.cpu().numpy(), float(cl), stats.cpu(), _flat_split(list(actors.parameters()) +
                                                                           list(critic.parameters()), probe[0])))
    (al0, cl0, st0, g0), (al1, cl1, st1, g1) = res
    print("actor", al0, al1, "critic", cl0, cl1, "kl", st0[:, 1].tolist(), st1[:, 1].tolist())
    assert float(st0[:, 1].abs().max()) > 0.0           # the policy moved in epoch 0: the ratio is live
    assert np.all(np.isfinite(al1)) and np.isfinite(cl1)
    assert np.allclose(al0, al1, rtol=1e-4, atol=1e-6)
    assert cl1 == pytest.approx(cl0, rel=1e-4)
    for x, y in zip(g0, g1):
        scale = float(x.abs().max()) + 1e-12
        assert float((x - y).abs().max()) <= 1e-3 * scale


def test_ppo_learner_end_to_end(M, tmp_path):
    A, PPO, V = M["A"], M["PPO"], M["V"]
    n, T = 128, 16
    learner = PPO.VecMultiAgentPPO(V.FJSPVecEnv(n), batch_size=T, ppo_epochs=3, seed=13)
    learner.learn(2 * T * n, num_orders=25, seeds=torch.arange(n))
    assert len(learner.ppo_history) == 2 * 3
    assert [(r["batch"], r["epoch"]) for r in learner.ppo_history] == [(i, k) for i in range(2) for k in range(3)]
    for r in learner.ppo_history:
        assert np.all(np.isfinite(r["actor_loss"])) and np.isfinite(r["critic_loss"])
        assert np.all(np.isfinite(r["entropy"])) and np.all(np.isfinite(r["clip_frac"]))
        if r["epoch"] == 0:
            assert r["kl"] == [0.0] * 8 and r["clip_frac"] == [0.0] * 8
        else:
            assert min(r["kl"]) >= 0.0
    assert len(learner.critic_loss_history) == 2
    assert learner.critic_loss_history[-1] == learner.ppo_history[-1]["critic_loss"]
    assert [learner.actor_loss_history[a][-1] for a in learner.possible_agents] == learner.ppo_history[-1]["actor_loss"]
    b = learner._bufs
    # step t acted on masks[t]; masks[0] was replaced by roll_over() after the last update
    acts = b["actions"][1:].long()
    masks = b["masks"][1:T]
    for a in range(8):
        chosen = masks[:, A.MASK_OFFS[a]:A.MASK_OFFS[a] + A.N_ACTIONS[a], :].gather(1, acts[:, a:a + 1, :])
        assert bool((chosen == 1).all()), a
    assert int(b["status"].bitwise_and(1).sum()) == 0
    path = str(tmp_path / "ppo.pt")
    learner.save_model(path)
    other = PPO.VecMultiAgentPPO(V.FJSPVecEnv(n), batch_size=T, seed=99)
    other.load_model(path)
    for i in range(8):
        for k, v in learner.actors.actor_state_dict(i).items():
            assert torch.equal(other.actors.actor_state_dict(i)[k], v), (i, k)
    for k, v in learner.critic.state_dict().items():
        assert torch.equal(other.critic.state_dict()[k], v), k
