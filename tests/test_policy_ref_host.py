"""The float64 policy reference (tests/policy_ref.py) itself, on the CPU: it equals the learner's
eager policy within f32 rounding and the trained fixture's recorded actions and values, its draw
equals sample_categorical away from the CDF steps, the fallback set's probabilities as constructed
from the masks are torch's f32 ones bit for bit, and every operand set of the GPU tests
(tests/test_gpu_policy_kernel.py) meets the preconditions and the excluded-share caps with torch's
f32 path standing in for the kernel."""
import pytest
import torch

from tests import policy_ref as R

A = R.A
N = 1000
SETS = ("i", "ii")


class _CpuEnv:
    def __init__(self, n):
        self.device, self.num_envs, self.env_id_base = torch.device("cpu"), n, 0


@pytest.fixture(scope="module")
def ref():
    """Per weight set: networks, the mixed operands, float64 and eager f32 results."""
    out = {}
    for kind in ("i", "ii", "iii"):
        actors, critic = R.networks(kind, 0)
        feats, masks = R.operands("mixed", N, 3)
        lg, pm, v = R.policy64(actors, critic, feats, masks)
        pm32, v32 = R.policy32(actors, critic, feats, masks)
        out[kind] = dict(actors=actors, critic=critic, feats=feats, masks=masks, lg=lg, pm=pm, v=v, pm32=pm32, v32=v32)
    return out


@pytest.mark.parametrize("kind", SETS)
def test_policy64_equals_the_eager_policy(ref, kind):
    r = ref[kind]
    L = A.VecMultiAgentA2C(_CpuEnv(N), batch_size=4, seed=0, use_graph=False)
    L.actors.load_state_dict(r["actors"].state_dict())
    L.critic.load_state_dict(r["critic"].state_dict())
    act, pm, v = L.policy(r["feats"], r["masks"], deterministic=True)
    assert torch.equal(pm, r["pm32"]) and torch.equal(v, r["v32"])           # policy32 is the learner's path
    assert float((pm.double() - r["pm"]).abs().max()) <= 5e-5
    assert float((v.double() - r["v"]).abs().max()) <= 5e-5
    b = R.bound((pm.double() - r["pm"]).abs().max())
    clear = R.top2_margin(r["pm"]) > 2 * b
    assert torch.equal(act[clear], torch.argmax(r["pm"], dim=1)[clear])
    assert float((~clear).float().mean()) <= R.NEAR_TIE_SHARE
    pad = torch.arange(8)[None, :, None] >= torch.tensor(A.N_ACTIONS)[:, None, None]
    assert bool((r["pm"][pad.expand_as(r["pm"])] == 0).all())


def test_policy64_on_the_trained_fixture():
    feats, masks, acts, vals = R.trained_states()
    actors, critic = R.networks("ii")
    lg, pm, v = R.policy64(actors, critic, feats, masks)
    R.preconditions(lg, masks)
    assert torch.equal(torch.argmax(pm, dim=1), acts.long())
    assert torch.allclose(v, vals.double(), rtol=1e-5, atol=0)


@pytest.mark.parametrize("kind", SETS)
def test_draw64_equals_sample_categorical_outside_the_radius(ref, kind):
    r = ref[kind]
    b = R.bound((r["pm32"].double() - r["pm"]).abs().max())
    rad = R.radius(b)
    mismatches = total = 0
    per_agent = torch.zeros(8)
    for seed, step, gid0 in R.draw_keys(N):
        act, dist = R.draw64(r["pm"], seed, gid0, step)
        gid = (gid0 + torch.arange(N)) & 0xFFFFFFFF
        act32 = A.sample_categorical(r["pm32"], A.counter_uniform(seed, gid, step, "cpu"))
        far = dist > rad
        mismatches += int((act != act32)[far].sum())
        per_agent += (~far).float().sum(dim=1)
        total += N
        # a draw never lands on an invalid or zero-probability action, excluded or not
        assert bool((r["pm"].gather(1, act[:, None]) > 0).all()) and bool((r["pm32"].gather(1, act32[:, None]) > 0).all())
    assert mismatches == 0
    assert float(per_agent.max()) / total <= R.DRAW_EXCLUDED_SHARE, per_agent / total      # each agent on its own


def test_draw64_keys_by_global_id_and_wraps():
    pm = torch.full((8, 8, 40), 0.125, dtype=torch.float64)
    a, _ = R.draw64(pm, 5, 2 ** 32 - 10, 2 ** 32 - 1)
    lo, _ = R.draw64(pm[:, :, :10], 5, 2 ** 32 - 10, 2 ** 32 - 1)
    hi, _ = R.draw64(pm[:, :, :30], 5, 0, 2 ** 32 - 1)
    assert torch.equal(a[:, :10], lo) and torch.equal(a[:, 10:], hi)
    assert len(torch.unique(a)) == 8
    # a zero-probability action in the middle of the CDF is never drawn, the last valid one is
    pm = torch.zeros(8, 8, 4000, dtype=torch.float64)
    pm[:, 0], pm[:, 2] = 0.5, 0.5
    a, dist = R.draw64(pm, 9, 0, 3)
    assert set(torch.unique(a).tolist()) == {0, 2} and abs(float((a == 2).float().mean()) - 0.5) < 0.02


def test_fallback_set_construction_is_torch_f32_bit_for_bit(ref):
    r = ref["iii"]
    gap = R.preconditions(r["lg"], r["masks"])
    exp, fb = R.fallback_probs(r["masks"])
    assert torch.equal(fb, gap >= R.GAP_FALLBACK) and bool((gap[~fb] == 0).all())
    assert 0.2 < float(fb.float().mean()) < 0.35
    m = A.agent_masks(r["masks"], A.mask_index("cpu"))
    k = m.sum(dim=1, keepdim=True)
    uni32 = torch.where(m > 0, (1.0 / k).expand_as(m), torch.zeros_like(m))     # exactly 1.0f / k on the valid actions
    exp32 = torch.where(fb[:, None, :], uni32, exp.float())
    assert torch.equal(r["pm32"], exp32)
    assert torch.equal(exp.float(), exp32)                                       # float64 1 / k rounds to 1.0f / k
    # float64 without special handling keeps 1e-100 where f32 keeps 0: no fallback there
    assert float((r["pm"] - exp)[fb[:, None, :].expand_as(exp)].abs().max()) > 0.1
    assert float((r["pm"] - exp)[~fb[:, None, :].expand_as(exp)].abs().max()) < 1e-100
    # greedy: the lowest valid index under the fallback, j0 elsewhere
    first = torch.argmax(m, dim=1)
    assert torch.equal(torch.argmax(r["pm32"], dim=1), torch.where(fb, first, torch.tensor(R.J0)[:, None].expand_as(first)))


# the operand sets of tests/test_gpu_policy_kernel.py: (weight sets, operand kind, n, operand seed)
GPU_OPERANDS = ([(("i", "ii", "iii"), "mixed", N, 3), (("iii",), "mixed", 3, 3)] + [(("i", "ii"), "dedup", n, 3) for n in (552, 532)] +
                [(("i",), "mixed", n, 3) for n in (1, 31, 32, 33, 63, 64, 65, 96, 129)] +
                [(("i",), "mixed", n, 10 + t) for n in (1, 33, 64, 65, 96) for t in range(4)])


@pytest.mark.parametrize("kinds,okind,n,opseed", GPU_OPERANDS)
def test_preconditions_and_caps_hold_for_every_gpu_operand_set(kinds, okind, n, opseed):
    """Every operand set is finite, keeps a valid action per agent and stays clear of the logit gaps
    at which f32 underflow decides; with torch's f32 path on the CPU standing in for the kernel, the
    shares excluded as near-ties (case A) and as draws next to a CDF step (case B) are under their
    caps, so a cap exceeded on the GPU is the kernel's doing."""
    feats, masks = R.operands(okind, n, opseed)
    assert feats.shape == (38, n) and masks.shape == (29, n) and bool(torch.isfinite(feats).all())
    for kind in kinds:
        actors, critic = R.networks(kind, 0)
        lg, pm, v = R.policy64(actors, critic, feats, masks)
        gap = R.preconditions(lg, masks)
        if kind == "iii":
            if n == N:
                R.preconditions(lg, R.force_tiles(masks, (0, 3, 6), range(0, 16, 2)))
            continue
        assert bool((gap <= R.GAP_SAME).all())
        pm32, _ = R.policy32(actors, critic, feats, masks)
        b = R.bound((pm32.double() - pm).abs().max())
        assert float((R.top2_margin(pm) <= 2 * b).float().mean()) <= R.NEAR_TIE_SHARE
        if opseed != 3:
            continue                                       # the step test's operands: no share is asserted
        near = total = 0
        for seed, step, gid0 in R.draw_keys(n):
            near += int((R.draw64(pm, seed, gid0, step)[1] <= R.radius(b)).sum())
            total += 8 * n
        assert near / total <= R.DRAW_EXCLUDED_SHARE


def test_dedup_operands_follow_the_plan():
    for n in (532, 552):
        feats, masks = R.operands("dedup", n, 3)
        plan = R.tile_distinct(n)
        assert plan[0][-1] == (33 if n == 552 else 5)
        seen = set()
        for a in range(2, 8):
            x = feats[A.OBS_OFFS[a]:A.OBS_OFFS[a] + 3]
            for t, k in enumerate(plan[a - 2]):
                cols = x[:, 64 * t:64 * t + 64].t()
                uniq, inv = torch.unique(cols, dim=0, return_inverse=True)
                assert len(uniq) == k
                if 1 < k < cols.shape[0]:
                    assert bool((inv[1:] != inv[:-1]).all()) or k < 31          # equal triples are not adjacent
                    first = {int(i): int((inv == i).nonzero()[0]) for i in inv.unique()}
                    assert sorted(first.values()) != list(range(k))              # leaders are not the first k lanes
                seen.add((a, k))
        assert all((a, k) in seen for a in range(2, 8) for k in R.DEDUP_KS)      # every station agent meets every k
        m = A.agent_masks(masks, A.mask_index("cpu"))
        per_tile = torch.nn.functional.pad(m.sum(dim=1), (0, -n % 64)).view(8, -1, 64).max(dim=2).values
        assert bool((per_tile >= 2).all())                                       # no tile is forced


def test_kernel_model_of_the_critic(ref):
    """policy_ref.critic_model, the critic by the kernel's arithmetic: the six plane products summed
    in float64 are within the 2^-22 |a b| of the three dropped products and the split residuals, far
    inside f32 rounding; with f32 accumulators the model is at torch's f32 level, and the small
    products in an accumulator of their own (critic_tile) cost less rounding than in the one."""
    r = ref["i"]
    scale = max(1.0, float(r["v"].abs().max()))
    e64 = float((R.critic_model(r["critic"], r["feats"]) - r["v"]).abs().max())
    f, v = r["feats"][:, :256], r["v"][:256]
    two = (R.critic_model(r["critic"], f, f32_acc=True) - v).abs()
    one = (R.critic_model(r["critic"], f, f32_acc=True, small_acc=False) - v).abs()
    assert e64 <= 2.0 ** -22 * scale, e64
    assert e64 < float(two.max()) <= 4 * float((r["v32"].double() - r["v"]).abs().max())
    assert float(two.mean()) < float(one.mean())
