"""The PPO learner (ppo_vec.py) on the CPU: the dense loss head and its gradient against the same
formulas restated in float64, epoch 0 against A2C, the grouped path against the dense one, the
epoch loop (target_kl, per-batch work done once) and the new entry's argument checks.

The clipped objective is an extension (the reference has A2C only), so the yardsticks are a
float64 restatement written out in tests/backward_ref.py and the A2C losses the project already
pins to the reference.  The GPU version (the HIP loss head) is tests/test_gpu_ppo.py."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tests import gpu_util as G
from tests.backward_ref import _oracle_batch, _reference_f64

A = importlib.import_module("multi-agent-rl-for-fjsp_amd.a2c_vec")
PPO = importlib.import_module("multi-agent-rl-for-fjsp_amd.ppo_vec")

EPS_CLIP = 0.2
# every ratio at least 1 % away from a clip bound (0.8, 1.2): f32 rounding cannot flip a sample
RATIOS = (0.5, 0.79, 0.9, 1.0, 1.1, 1.21, 1.6)


def _params(actors, critic):
    return list(actors.parameters()) + list(critic.parameters())


def _constructed_logp_old(actors, feats, masks, acts, gidx, midx, seed=23):
    """logp_now - log(r*) with r* drawn per (agent, sample) from RATIOS."""
    T, _, N = feats.shape
    with torch.no_grad():
        pm = A.masked_probs(actors(A.actor_inputs(feats, gidx)), A.agent_masks(masks, midx))
        logp = A.categorical_log_prob(pm, acts.long().permute(1, 0, 2).reshape(8, T * N))
    gen = torch.Generator().manual_seed(seed)
    rstar = torch.tensor(RATIOS)[torch.randint(0, len(RATIOS), logp.shape, generator=gen)]
    return (logp - torch.log(rstar)).contiguous()


def test_dense_loss_and_gradient_match_float64():
    feats, masks, acts, ret, adv = _oracle_batch()
    gidx, midx = A.gather_index("cpu"), A.mask_index("cpu")
    actors, critic = A.init_networks(seed=3)
    batch = PPO.PPOBatch(feats, masks, acts, ret, adv, gidx, midx, dedup=False)
    batch.logp_old = _constructed_logp_old(actors, feats, masks, acts, gidx, midx)
    ref = _reference_f64(actors, critic, feats, masks, acts, ret, adv, batch.mean, batch.std, batch.logp_old,
                         0.01, EPS_CLIP)
    cases = torch.stack(ref["cases"]).sum(0)
    assert bool((cases > 0).all()), cases.tolist()      # all five (sign of adv, clip side) cases occur
    al, stats = PPO.ppo_actor_losses(actors, batch, 0.01, EPS_CLIP)
    cl = batch.critic_loss(critic)
    (al.sum() + cl).backward()
    print("actor losses", al.tolist(), ref["loss"], "critic", cl.item(), ref["critic"])
    print("kl sums", stats[:, 1].tolist(), ref["kl"], "clip", stats[:, 2].tolist(), ref["clip"])
    assert np.allclose(al.detach().numpy(), ref["loss"], rtol=1e-4, atol=1e-6)
    assert cl.item() == pytest.approx(ref["critic"], rel=1e-4, abs=1e-6)
    assert np.allclose(stats[:, 0].numpy(), ref["ent"], rtol=1e-4, atol=1e-6)
    assert np.allclose(stats[:, 1].numpy(), ref["kl"], rtol=1e-4, atol=1e-6)
    assert stats[:, 2].long().tolist() == ref["clip"]
    for (name, p), g in zip(list(actors.named_parameters()) + list(critic.named_parameters()), ref["grads"]):
        err, scale = float((p.grad.double() - g).abs().max()), float(g.abs().max())
        print(name, "grad err", err, "scale", scale)
        assert err <= 1e-4 * scale, name


def test_epoch0_gradient_is_a2c():
    """The ratio to the policy's own log-probabilities is exactly 1: the PPO gradient is
    A2CLosses.compute's on the same batch, in record mode and with the recorded logp_old given."""
    feats, masks, acts, ret, adv = _oracle_batch()
    gidx, midx = A.gather_index("cpu"), A.mask_index("cpu")
    actors, critic = A.init_networks(seed=4)
    batch = PPO.PPOBatch(feats, masks, acts, ret, adv, gidx, midx, dedup=False)
    al, cl = A.A2CLosses.compute(actors, critic, feats, masks, acts, ret, adv, gidx, midx, 0.01, batch.mean, batch.std,
                                 batch.count)
    (al.sum() + cl).backward()
    want = [p.grad.clone() for p in _params(actors, critic)]
    for mode in ("record", "given"):
        for p in _params(actors, critic):
            p.grad = None
        pl, stats = PPO.ppo_actor_losses(actors, batch, 0.01, EPS_CLIP)
        assert batch.logp_old is not None
        (pl.sum() + batch.critic_loss(critic)).backward()
        # (the loss values differ: -sum adv_n r with r = 1 against -sum adv_n logp; the gradients agree)
        assert float(stats[:, 1].abs().max()) == 0.0 and float(stats[:, 2].abs().max()) == 0.0, mode
        for p, w in zip(_params(actors, critic), want):
            assert float((p.grad - w).abs().max()) <= 1e-6 * float(w.abs().max()), mode


def _synthetic_batch():
    """test_grouped_update_equals_dense_update's batch: many repeated observations."""
    T, N = 16, 64
    gen = torch.Generator().manual_seed(5)
    feats = torch.randint(0, 3, (T, A.GLOBAL_DIM, N), generator=gen).float()
    feats[:, 5:9] = torch.randint(0, 40, (T, 4, N), generator=gen).float()
    feats[:, 21] = torch.rand(T, N, generator=gen).round(decimals=1)
    masks = torch.randint(0, 2, (T, 29, N), generator=gen).to(torch.int8)
    masks[:, A.MASK_OFFS] = 1
    acts = torch.stack([torch.randint(0, n, (T, N), generator=gen) for n in A.N_ACTIONS], 1).to(torch.uint8)
    ret = torch.randn(T, A.NA, N, generator=gen, dtype=torch.float64)
    adv = torch.randn(T, A.NA, N, generator=gen, dtype=torch.float64)
    return feats, masks, acts, ret, adv


def test_grouped_ppo_equals_dense_ppo():
    """Three epochs grouped (each network once per distinct input) and dense from the same start:
    the same losses, statistics and parameter steps, summed in another order
    (test_grouped_update_equals_dense_update's tolerances).  Plain SGD, so that a parameter's
    step is its gradient (Adam's first steps are ~lr sign(grad), which turns rounding of a
    near-zero gradient into a full step); lr 0.01: with features up to 40 the gradients' entries
    reach ~0.1, so a step moves a weight by <= ~1e-3, the order of the learner's Adam steps, and the
    three epochs stay a PPO-sized policy change (that test's single step uses lr 1.0, which here
    would move weights by thousands before the second epoch and compare nothing but overflow)."""
    feats, masks, acts, ret, adv = _synthetic_batch()
    gidx, midx = A.gather_index("cpu"), A.mask_index("cpu")
    res = []
    for dedup in (False, True):
        actors, critic = A.init_networks(seed=11)
        oa = torch.optim.SGD(actors.parameters(), lr=0.01)
        oc = torch.optim.SGD(critic.parameters(), lr=0.01)
        before = [p.detach().clone() for p in _params(actors, critic)]
        recs = PPO.ppo_update(actors, critic, oa, oc, feats, masks, acts, ret, adv, gidx, midx, 0.01, 1e9, 3, EPS_CLIP,
                              dedup=dedup)
        res.append((recs, [b - p.detach() for p, b in zip(_params(actors, critic), before)]))
    (r0, g0), (r1, g1) = res
    assert len(r0) == len(r1) == 3
    for k, (x, y) in enumerate(zip(r0, r1)):
        print(k, x["actor_loss"], y["actor_loss"], x["kl"], y["kl"], x["clip_frac"], y["clip_frac"])
        assert np.allclose(x["actor_loss"], y["actor_loss"], rtol=1e-5, atol=1e-6), k
        assert y["critic_loss"] == pytest.approx(x["critic_loss"], rel=1e-5), k
        assert np.allclose(x["entropy"], y["entropy"], rtol=1e-5, atol=1e-6), k
        assert np.allclose(x["kl"], y["kl"], rtol=1e-5, atol=1e-6), k
    assert max(r0[2]["kl"]) > 0.0
    for a, b in zip(g0, g1):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-6)


def _adam_learner(seed):
    actors, critic = A.init_networks(seed=seed)
    return actors, critic, torch.optim.Adam(actors.parameters(), lr=3e-4), torch.optim.Adam(critic.parameters(), lr=1e-3)


def test_target_kl_stops_and_epochs_move_parameters():
    feats, masks, acts, ret, adv = _oracle_batch()
    gidx, midx = A.gather_index("cpu"), A.mask_index("cpu")
    actors, critic, oa, oc = _adam_learner(6)
    recs = PPO.ppo_update(actors, critic, oa, oc, feats, masks, acts, ret, adv, gidx, midx, 0.01, 0.5, 5, EPS_CLIP,
                          target_kl=0.0)
    assert len(recs) == 2                           # epoch 0's KL is exactly 0, epoch 1's is not
    assert recs[0]["kl"] == [0.0] * 8 and recs[0]["clip_frac"] == [0.0] * 8
    assert float(np.mean(recs[1]["kl"])) > 0.0
    actors, critic, oa, oc = _adam_learner(6)
    snaps = []
    recs = PPO.ppo_update(actors, critic, oa, oc, feats, masks, acts, ret, adv, gidx, midx, 0.01, 0.5, 3, EPS_CLIP,
                          grad_probe=lambda g: snaps.append([p.detach().clone() for p in _params(actors, critic)]))
    assert len(recs) == 3 and len(snaps) == 3
    snaps.append([p.detach().clone() for p in _params(actors, critic)])
    for k in range(3):                              # every epoch's Adam step moved both networks
        assert any(not torch.equal(x, y) for x, y in zip(snaps[k][:6], snaps[k + 1][:6])), k
        assert any(not torch.equal(x, y) for x, y in zip(snaps[k][6:], snaps[k + 1][6:])), k
    for r in recs:
        assert set(r) == {"actor_loss", "critic_loss", "entropy", "kl", "clip_frac"}
        assert len(r["actor_loss"]) == len(r["entropy"]) == len(r["kl"]) == len(r["clip_frac"]) == 8
        assert np.all(np.isfinite(r["actor_loss"])) and np.isfinite(r["critic_loss"])
    with pytest.raises(ValueError):
        PPO.ppo_update(actors, critic, oa, oc, feats, masks, acts, ret, adv, gidx, midx, 0.01, 0.5, 3, 1.0)


def test_per_batch_work_is_done_once(monkeypatch):
    """A 4-epoch update computes the keys and verifies the grouping once, not once per epoch."""
    feats, masks, acts, ret, adv = _synthetic_batch()
    gidx, midx = A.gather_index("cpu"), A.mask_index("cpu")
    calls = {"keys": 0, "verify": 0}
    keys, verify = A.group_keys, A.group_verify

    def count_keys(*a, **k):
        calls["keys"] += 1
        return keys(*a, **k)

    def count_verify(*a, **k):
        calls["verify"] += 1
        return verify(*a, **k)
    monkeypatch.setattr(A, "group_keys", count_keys)
    monkeypatch.setattr(A, "group_verify", count_verify)
    actors, critic, oa, oc = _adam_learner(7)
    recs = PPO.ppo_update(actors, critic, oa, oc, feats, masks, acts, ret, adv, gidx, midx, 0.01, 0.5, 4, EPS_CLIP)
    assert len(recs) == 4
    assert calls == {"keys": 1, "verify": 1}


def test_ppo_head_validates_arguments_without_gpu():
    """fjsp_a2c_actor_head_ppo rejects null buffers, empty shapes and a clip range outside (0, 1)
    before launching; logp_old / logp_out may be null (record mode / no output)."""
    L = G.native.lib()
    P = ctypes.c_void_p
    a = P(1 << 20)
    ok = [a, 8, a, 4, 4, a, a, a, a, a, a, a, 0.2, 1.0, 0.01, a, a, None]

    def bad(i, v, msg):
        b = list(ok)
        b[i] = v
        assert L.fjsp_a2c_actor_head_ppo(*b) != 0 and msg in L.fjsp_last_error(), (i, v)
    for i in (0, 2, 5, 6, 7, 15, 16):
        bad(i, None, b"null")
    bad(8, None, b"null")                           # adv_mean without adv_std
    bad(3, 0, b"must be > 0")
    bad(4, 0, b"must be > 0")
    bad(1, 0, b"must be > 0")
    for eps in (0.0, 1.0, -0.1, 1.5, float("nan")):
        bad(12, eps, b"clip_eps")
    assert L.fjsp_abi_version() == 14


def test_learner_constructor_checks():
    """Sharded or gathered PPO is not built: a process group is refused at construction."""
    class Env:
        device, num_envs = torch.device("cpu"), 4
    with pytest.raises(NotImplementedError):
        PPO.VecMultiAgentPPO(Env(), group=object())
    with pytest.raises(ValueError):
        PPO.VecMultiAgentPPO(Env(), ppo_clip=1.0)
    learner = PPO.VecMultiAgentPPO(Env(), batch_size=8, seed=1, ppo_epochs=2)
    assert (learner.ppo_epochs, learner.ppo_clip, learner.target_kl, learner.ppo_history) == (2, 0.2, None, [])
