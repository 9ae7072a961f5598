"""tests/backward_ref.py on the CPU: the masked float64 backward against float64 autograd, the
decidedness bound against an f32 forward, the conditions on the inputs that
tests/test_gpu_backward_edges.py runs on, and the update batches' f32 twin (the dense CPU update)
against the float64 restatement, so that a miss on the GPU is the GPU path's."""
import copy

import pytest
import torch

from tests import backward_ref as R

A = R.A


def _rel(got, want):
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("U", [1, 33, 97])
def test_masked_backward_equals_float64_autograd(kind, U):
    """critic_backward64 with the masks z > 0 == float64 autograd of sum a / 2 V^2 + b V + c through
    critic.net.double(), to 1e-12 relative: the pre-activation gradients g1, g2, g3 (autograd's
    gradients of the Linear outputs), the values, the loss, and the eight parameter gradients (the
    tile partial sums added over the tiles, g^T x for the weights)."""
    critic, x, coef = R.critic_operands(kind, U)
    z1, z2, z3, v = R.critic_forward64(critic, x)
    r = R.critic_backward64(critic, x, coef, z1 > 0, z2 > 0, z3 > 0)
    net = copy.deepcopy(critic.net).double()
    h, zs = x.double(), []
    for m in net:
        h = m(h)
        if isinstance(m, torch.nn.Linear):
            h.retain_grad()
            zs.append(h)
    V = h.reshape(-1)
    loss = (0.5 * coef[:, 0] * V * V + coef[:, 1] * V + coef[:, 2]).sum()
    loss.backward()
    loss = loss.detach()
    assert _rel(v, V.detach()) <= 1e-12
    assert abs(float(r["loss"].sum()) - float(loss)) <= 1e-12 * abs(float(loss))
    assert r["loss"].shape == (-(-U // 32),) and r["part"].shape == (-(-U // 32), R.PW)
    for name, z in (("g1", zs[0]), ("g2", zs[1]), ("g3", zs[2])):
        assert _rel(r[name], z.grad) <= 1e-12, name
    assert _rel(r["gv"], zs[3].grad.reshape(-1)) <= 1e-12
    for got, p in zip(R.param_grads(r, x.double()), net.parameters()):
        assert got.shape == p.grad.shape
        assert _rel(got, p.grad) <= 1e-12
    assert bool((r["part"][:, 769:] == 0).all())
    # the padding state contributes nothing
    s = R.padding_state(U)
    assert float(coef[s].abs().max()) == 0.0
    assert all(float(r[k][s].abs().max()) == 0.0 for k in ("g1", "g2", "g3"))


def test_tile_sums_are_per_tile():
    """part / loss rows are sums over their own tile's states only: the rows of a 97-state case
    equal those of the same states evaluated tile by tile."""
    critic, x, coef = R.critic_operands("init", 97)
    z1, z2, z3, _ = R.critic_forward64(critic, x)
    r = R.critic_backward64(critic, x, coef, z1 > 0, z2 > 0, z3 > 0)
    for t, lo in enumerate(range(0, 97, 32)):
        s = slice(lo, min(lo + 32, 97))
        one = R.critic_backward64(critic, x[s], coef[s], (z1 > 0)[s], (z2 > 0)[s], (z3 > 0)[s])
        assert _rel(r["part"][t], one["part"][0]) <= 1e-13
        assert abs(float(r["loss"][t] - one["loss"][0])) <= 1e-13 * abs(float(one["loss"][0]))


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("U", R.CRITIC_U)
def test_input_conditions_hold(kind, U):
    """The conditions the GPU test relies on, for its weights, seeds and every U (it asserts them
    again): few undecided units, none on a tile's first or last state, mixed masks."""
    critic, x, coef = R.critic_operands(kind, U)
    share, d = R.critic_conditions(critic, x)
    print(f"BACKWARD_EDGES conditions kind={kind} U={U} undecided_share={share:.2e}")
    assert x.shape == (U, 38) and coef.shape == (U, 3)
    s = R.padding_state(U)
    assert float(coef[s].abs().max()) == 0.0 and int((coef.abs().sum(1) == 0).sum()) == 1
    # a state's operands do not depend on the launch: the tile-independence test compares launches
    _, x97, c97 = R.critic_operands(kind, 97)
    assert torch.equal(x, x97[:U]) and (U < 32 or torch.equal(coef, c97[:U]))


@pytest.mark.parametrize("kind", ["init", "trained"])
def test_decided_bound_holds_for_an_f32_forward(kind):
    """An f32 forward (torch on the CPU) stays inside the bound at every unit, so every decided
    unit's ReLU comes out as in float64; and the f32 yardstick is the float64 backward's formulas
    (its results agree to f32 level under the same masks)."""
    critic, x, coef = R.critic_operands(kind, 97)
    z64 = R.critic_forward64(critic, x)
    e = R.decided_bounds(critic, x)
    with torch.no_grad():
        z32 = R._forward(R.critic_params(critic, torch.float32), x)
    for l in range(3):
        assert bool(((z32[l].double() - z64[l]).abs() <= e[l]).all()), l
        d = z64[l].abs() > e[l]
        assert bool(((z32[l] > 0) == (z64[l] > 0))[d].all()), l
    m = [z > 0 for z in z32[:3]]
    r64 = R.critic_backward64(critic, x, coef, *m)
    r32 = R.critic_backward32(critic, x, coef, *m, device="cpu")
    for k in ("h1", "h2", "values", "g3", "g2", "g1", "part", "loss"):
        assert r32[k].shape == r64[k].shape
        assert _rel(r32[k].double(), r64[k]) <= 1e-4, k


@pytest.mark.parametrize("name", list(R.UPDATE_BATCHES))
def test_dense_cpu_update_meets_the_update_bounds(name):
    """The reference's own f32 twin: the dense CPU update (A2CLosses.compute without dedup) against
    _reference_f64 with ratio 1 on each batch of the GPU test, under the bounds that test uses."""
    actors, critic, batch, count, mean, std, ref = R.update_case(name)
    assert ref["kl"] == [0.0] * 8 and ref["clip"] == [0] * 8          # every ratio exactly 1
    gidx, midx = A.gather_index("cpu"), A.mask_index("cpu")
    z = torch.zeros(8)
    al, cl = A.A2CLosses.compute(actors, critic, *batch, gidx, midx, 0.01, z if mean is None else mean,
                                 z if std is None else std, count, dedup=False)
    (al.sum() + cl).backward()
    params = list(actors.named_parameters()) + list(critic.named_parameters())
    R.check_update(al.tolist(), cl.item(), [p.grad for _, p in params], ref, [k for k, _ in params],
                   report=lambda **kw: print("BACKWARD_EDGES update", name, kw))
