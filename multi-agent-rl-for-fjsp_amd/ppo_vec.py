"""Batched multi-agent PPO over N device-resident environments: clipped multi-epoch updates on the
grouped A2C path.

An extension: the reference (a2c.py) has A2C only, one Adam step per collected batch.  PPO spends
the same batch on several epochs, kept honest by the clipped probability ratio to the policy that
collected it.  Everything but the loss is a2c_vec's: the networks, the masked probabilities and
uniform fallback (a2c.py:204-220), the entropy bonus and per-agent advantage normalisation
(a2c.py:705-731), the critic's MSE against the fixed returns (a2c.py:713-722), the per-agent
gradient clipping and Adam (a2c.py:675-679).

  * per (agent, sample): r = exp(logp - logp_old), surr = min(r adv_n, clamp(r, 1 - eps, 1 + eps)
    adv_n); actor_loss_a = -(sum surr) / count - c (sum entropy) / count;
  * the behaviour policy's log-probabilities are recorded by the update's own first forward (the
    weights that collected the batch), so the first epoch's ratio is exactly 1 and its gradient is
    A2C's;
  * the grouped update's fixed costs depend on the batch's features alone, so they are paid once
    per batch (PPOBatch, the A2C update's a2c_vec.UpdateBatch kept over the epochs): advantage
    statistics, key pass, grouping and verification, the groups' representative rows, the
    critic's loss coefficients.  Every epoch reuses them: forward -> losses -> backward ->
    a2c_vec.clip_and_step;
  * on the GPU with a verified grouping the loss head is one HIP kernel (fjsp_a2c_actor_head_ppo:
    the A2C head's kernel, k_actor_head in csrc/fjsp_policy.hip, instantiated with the ratio and
    clip as its dL / dlogp); everywhere else (the CPU, dedup=False, a hash collision) it is the
    torch ops of ppo_head_terms, the readable specification.

Out of scope: minibatches (a subset of a group's samples would need per-sample weights in the run
sums), value-loss clipping, graph capture of the update, multi-GPU exchanges.
"""
import numpy as np
import torch

from . import a2c_vec as A
from .a2c_vec import NA
from .spec import AGENTS


def clip_bounds(clip_eps):
    """(1 - eps, 1 + eps) rounded as the kernel computes them: f32 arithmetic on the f32 eps."""
    e = np.float32(clip_eps)
    return float(np.float32(1.0) - e), float(np.float32(1.0) + e)


def ppo_head_terms(probs, m, acts, adv_n, logp_old, clip_eps):
    """The PPO loss head per (agent, sample) in torch ops.  probs [8, 8, S] (the actors' outputs
    per sample), m [8, 8, S] float masks, acts long [8, S], adv_n f32 [8, S] (normalised),
    logp_old f32 [8, S] or None (record mode: the current log-probabilities, detached: ratio 1)
    -> (surr, entropy, kl term (r - 1) - (logp - logp_old), clipped (bool), logp), each [8, S]."""
    ent = A.entropy_of(probs)
    logp = A.categorical_log_prob(A.masked_probs(probs, m), acts)
    old = logp.detach() if logp_old is None else logp_old
    d = logp - old
    r = torch.exp(d)
    lo, hi = clip_bounds(clip_eps)
    surr = torch.minimum(r * adv_n, torch.clamp(r, lo, hi) * adv_n)
    clipped = ((adv_n > 0) & (r > hi)) | ((adv_n < 0) & (r < lo))
    return surr, ent, (r - 1.0) - d, clipped, logp


class _ActorHeadPPO(torch.autograd.Function):
    """a2c_vec._ActorHead for the clipped objective, over the same launch helper
    (a2c_vec.actor_head_forward with the three PPO operands: fjsp_a2c_actor_head_ppo).  Also returns
    stats f64 [8, 3] = per agent the sums of the entropy, of the KL terms and the number of clipped
    samples (not differentiable)."""

    @staticmethod
    def forward(ctx, pu, g, masks, actions, adv, adv_mean, adv_std, logp_old, logp_out, clip_eps, count, coef):
        losses, sums = A.actor_head_forward(ctx, pu, g, masks, actions, adv, adv_mean, adv_std, count, coef,
                                            (logp_old, logp_out, clip_eps))
        stats = sums[:, 1:].contiguous()
        ctx.mark_non_differentiable(stats)
        return losses, stats

    @staticmethod
    def backward(ctx, gl, _gstats):
        return A.actor_head_backward(ctx, gl, 12)


class PPOBatch(A.UpdateBatch):
    """a2c_vec.UpdateBatch kept over several epochs, with the batch's own advantage statistics,
    the behaviour policy's log-probabilities and the clipped loss head.  actor_losses() and
    critic_loss() are one epoch's forward; the first epoch gathers the groups' representatives,
    the later ones reuse them.

    logp_old f32 [8, T*N]: None until the first actor_losses() call, which runs in record mode and
    keeps the log-probabilities of its own forward (callers may set it: a batch resumed from a
    recorded state)."""

    def __init__(self, feats, masks, actions, ret, adv, gidx, midx, dedup=True):
        from . import distributed as D
        count, mean, std = D.adv_stats_slab(adv)                      # of FloatTensor(adv), a2c.py:724-731
        super().__init__(feats, masks, actions, ret, adv, gidx, midx, dedup, mean, std, count)
        self.logp_old = None

    def actor_losses(self, actors, entropy_coef, clip_eps):
        """Per agent -sum surr / count - entropy_coef sum entropy / count -> (losses f32 [8], stats
        f64 [8, 3] = per agent the sums of the entropy, of the KL terms and the number of clipped
        samples): the HIP loss head on the GPU with a verified grouping, the torch ops of
        ppo_head_terms everywhere else.  The first call records logp_old."""
        record = self.logp_old is None
        count = float(self.count)
        probs = self.actor_probs(actors)
        if self.head_kernel:
            buf = torch.empty(NA, self.S, dtype=torch.float32, device=probs.device) if record else None
            losses, stats = _ActorHeadPPO.apply(probs, self.ga, self.masks, self.actions, self.adv, *self.head_stats(),
                                                self.logp_old, buf, float(clip_eps), count, float(entropy_coef))
            if record:
                self.logp_old = buf
            return losses, stats
        surr, ent, kl, clipped, logp = ppo_head_terms(probs, *self.dense_operands(), self.logp_old, clip_eps)
        if record:
            self.logp_old = logp.detach().clone()
        losses = -surr.sum(dim=1) / count - entropy_coef * ent.sum(dim=1) / count
        stats = torch.stack([ent.detach().sum(dim=1), kl.detach().sum(dim=1), clipped.sum(dim=1).to(ent.dtype)],
                            dim=1).double()
        return losses, stats


def ppo_actor_losses(actors, batch, entropy_coef, clip_eps):
    """PPOBatch.actor_losses, as a function of the actors (tests/test_ppo_learner.py calls it)."""
    return batch.actor_losses(actors, entropy_coef, clip_eps)


def ppo_epoch(batch, actors, critic, optim_actor, optim_critic, entropy_coef, max_grad_norm, clip_eps,
              grad_probe=None):
    """One epoch over a PPOBatch: forward -> losses -> backward -> a2c_vec.clip_and_step.  Returns
    device tensors (no host synchronisation): actor losses [8], critic loss [1], stats [8, 3]
    (sums: entropy, KL terms, clipped samples)."""
    optim_actor.zero_grad(set_to_none=True)
    optim_critic.zero_grad(set_to_none=True)
    critic_loss = batch.critic_loss(critic)   # the critic first, as A2CLosses.compute
    actor_losses, stats = ppo_actor_losses(actors, batch, entropy_coef, clip_eps)
    (actor_losses.sum() + critic_loss).backward()
    A.clip_and_step(actors, critic, optim_actor, optim_critic, max_grad_norm, grad_probe)
    return actor_losses.detach(), critic_loss.detach().reshape(1), stats


def ppo_update(actors, critic, optim_actor, optim_critic, feats, masks, actions, ret, adv, gidx, midx,
               entropy_coef, max_grad_norm, epochs, clip_eps, target_kl=None, dedup=True, grad_probe=None,
               stage=None):
    """`epochs` clipped updates over one [T, ., N] batch (layouts as a2c_vec.update_step; works on
    CPU tensors).  The per-batch work (PPOBatch) is done once; epoch 0 runs the loss head in record
    mode (ratio 1: A2C's gradient) and its log-probabilities are logp_old for the rest.
    grad_probe(flat f32 grads) is called each epoch before clipping.  target_kl: after each epoch
    the mean over agents of sum kl / count is read (one host read per epoch, made only when
    target_kl is set) and the loop stops once it exceeds target_kl.  stage(name): called after the
    per-batch work ("prepare") and after each epoch ("epoch<k>") (timing marks).
    Returns one record per epoch run: {"actor_loss": [8], "critic_loss": float, "entropy": [8],
    "kl": [8], "clip_frac": [8]} (means over the batch's samples)."""
    if not 0.0 < float(clip_eps) < 1.0:
        raise ValueError("clip_eps must be in (0, 1)")
    if int(epochs) < 1:
        raise ValueError("epochs must be >= 1")
    batch = PPOBatch(feats, masks, actions, ret, adv, gidx, midx, dedup)
    if stage is not None:
        stage("prepare")
    out = []
    for k in range(int(epochs)):
        al, cl, stats = ppo_epoch(batch, actors, critic, optim_actor, optim_critic, entropy_coef, max_grad_norm,
                                  clip_eps, grad_probe)
        out.append(torch.cat([al.double(), cl.double(), (stats / batch.count).t().reshape(-1)]))
        if stage is not None:
            stage(f"epoch{k}")
        if target_kl is not None and float(out[-1][2 * NA + 1:3 * NA + 1].mean()) > target_kl:
            break
    rec = torch.stack(out).cpu().tolist()                             # the one host copy
    return [{"actor_loss": r[:NA], "critic_loss": r[NA], "entropy": r[NA + 1:2 * NA + 1],
             "kl": r[2 * NA + 1:3 * NA + 1], "clip_frac": r[3 * NA + 1:4 * NA + 1]} for r in rec]


class VecMultiAgentPPO(A.VecMultiAgentA2C):
    """VecMultiAgentA2C whose update is ppo_update: ppo_epochs clipped epochs per collected batch.
    collect, learn, test, episode tracking and checkpoints are inherited.  Single process only."""

    def __init__(self, env, *args, ppo_epochs=4, ppo_clip=0.2, target_kl=None, **kwargs):
        super().__init__(env, *args, **kwargs)
        if self.group is not None:
            raise NotImplementedError("VecMultiAgentPPO is single-process: sharded or gathered PPO is not built")
        if int(ppo_epochs) < 1:
            raise ValueError("ppo_epochs must be >= 1")
        if not 0.0 < float(ppo_clip) < 1.0:
            raise ValueError("ppo_clip must be in (0, 1)")
        self.ppo_epochs, self.ppo_clip = int(ppo_epochs), float(ppo_clip)
        self.target_kl = None if target_kl is None else float(target_kl)
        self.ppo_history = []      # every epoch's record (ppo_update), with its batch and epoch index
        self.ppo_stage = None      # stage(name) timing marks of ppo_update (scripts/ppo_epochs.py)
        self._ppo_batches = 0

    def update(self, ret=None, adv=None):
        """ppo_update over the rollout slab in place, then one repack(); the last epoch's losses go
        to the loss histories, every epoch's record to ppo_history."""
        fw = self.env.faults()     # synchronises
        if fw:
            raise RuntimeError(f"fjsp step kernels reported fault word {fw:#x} (a hand-off wait gave up): "
                               "the batch's transitions are invalid")
        t0 = self._start()
        if ret is None:
            ret, adv = self.advantages()
        b = self._bufs
        T = self.batch_size
        recs = ppo_update(self.actors, self.critic, self.optim_actor, self.optim_critic, b["feats"][:T],
                          b["masks"][:T], b["actions"], ret, adv, self.gidx, self.midx, self.entropy_coef,
                          self.max_grad_norm, self.ppo_epochs, self.ppo_clip, self.target_kl, self.dedup,
                          self.grad_probe, self.ppo_stage)
        self._mark("learn", t0)
        for k, r in enumerate(recs):
            self.ppo_history.append(dict(r, batch=self._ppo_batches, epoch=k))
        self._ppo_batches += 1
        al, cl = recs[-1]["actor_loss"], recs[-1]["critic_loss"]
        for a, x in zip(AGENTS, al):
            self.actor_loss_history[a].append(x)
        self.critic_loss_history.append(cl)
        self.repack()
        return al, cl
