"""The critic's backward kernels (csrc/fjsp_policy.hip) against float64 at their tile edges, and the
grouped update against the float64 restatement of the whole update (tests/backward_ref.py):

  fjsp_a2c_relu_bias_grad, fjsp_a2c_value_head_grad  element-wise outputs bit for bit, every word of
      the per-block sums within the a-priori bound of a 128-term f32 sum, around the rows a pass
      covers and the 128-row block;
  fjsp_a2c_critic_fused  every per-state output and every per-tile word at U = 1 .. 97 under the
      kernel's own ReLU masks (which must equal float64's at every decided unit), within 3 x the
      error of the same formulas in torch f32 on the same device + 2^-23 max |ref|; tiles bit-equal
      across launches; the eight parameter gradients through critic_onepass;
  fjsp_a2c_wgrad  where its split changes (stages = workgroups +- 1, few workgroups), every row;
  A2CLosses.compute(dedup=True) + backward  against _reference_f64 with ratio 1.

Every output of a direct C call lies in a larger buffer of NaN sentinels with guard words on both
sides.  Each case prints its figures (a line starting BACKWARD_EDGES) before it asserts; the
measured ones are in profiles/backward_edges/README.md."""
import copy
import ctypes
import json

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from tests import backward_ref as R  # noqa: E402

A = R.A
U32 = R.U32
GUARD = 1024                  # sentinel words on either side of an output (16-byte alignment kept)
FMIN = 2.0 ** -126            # the smallest positive normal f32
DENORM = 2.0 ** -140          # a positive denormal
UNDERFLOW = 2.0 ** -149       # an f32 product may round by half of this whatever its size


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from tests import gpu_util  # noqa: F401
    return {"nat": A.nat, "fused": {}}


def _report(**kw):
    print("BACKWARD_EDGES " + json.dumps(kw, sort_keys=True))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


class Guarded:
    """An output of `valid` leading rows inside a [rows, ...] view of NaN sentinels (rows > valid),
    itself between two guard regions of sentinels."""

    def __init__(self, shape, valid, dtype=torch.float32):
        numel = 1
        for d in shape:
            numel *= d
        assert shape[0] > valid
        self.valid = valid
        self.buf = torch.full((2 * GUARD + numel,), float("nan"), dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + numel].view(*shape)

    def check(self):
        """Guards and the rows past `valid` untouched, every word of the valid rows written ->
        the valid rows on the CPU."""
        assert bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[-GUARD:]).all())
        assert bool(torch.isnan(self.view[self.valid:]).all())
        out = self.view[:self.valid].cpu()
        assert not bool(torch.isnan(out).any())
        return out


# ---------------------------------------------------------------- the two element-wise kernels
def _rows_list(cols):
    rp = 1024 // cols                                  # rows one pass of the 256 threads covers
    return sorted({1, rp - 1, rp, rp + 1, 127, 128, 129, 256, 259})


EDGE_VALUES = (0.0, -0.0, -1.5, FMIN, DENORM)


def _edge_rows(rows):
    full = (rows // 128) * 128 - 1                     # the last row of the last full block
    return sorted({0, rows - 1} | ({full} if full >= 0 else set()))


def _edge_cols(cols):
    return (1, 5, 63, 64, cols - 1)


def _relu_operands(rows, cols, seed):
    """(gy, y) f32 [rows, cols] on the CPU: y a ReLU'd normal draw (about half zeros) with +0.0,
    -0.0, a negative, the smallest normal and a denormal in the first row, the last row and the
    last row of the last full block."""
    g = torch.Generator().manual_seed(seed)
    y = torch.relu(torch.randn(rows, cols, generator=g))
    gy = torch.randn(rows, cols, generator=g)
    for r in _edge_rows(rows):
        for c, v in zip(_edge_cols(cols), EDGE_VALUES):
            y[r, c] = v
    assert float(y[0, _edge_cols(cols)[4]]) == DENORM and 0 < float(y[0, _edge_cols(cols)[3]]) == FMIN
    assert rows * cols < 1024 or 0.4 < float((y == 0).float().mean()) < 0.6
    return gy, y


def _block_sums(t64, blocks):
    """f64 [rows, C] -> per 128-row block the column sums and the column sums of the magnitudes."""
    pad = blocks * 128 - t64.shape[0]
    t = torch.cat([t64, t64.new_zeros(pad, t64.shape[1])]) if pad else t64
    t = t.reshape(blocks, 128, -1)
    return t.sum(1), t.abs().sum(1)


@pytest.mark.parametrize("cols", [128, 256])
def test_relu_bias_grad_edges(M, cols):
    """g bit-equal to where(y > 0, gy, 0) (a denormal y passes, -0.0 and a negative do not, as
    aten's threshold_backward decides); every word of part[block] within 128 u sum |g| of the
    float64 column sum of that block's rows (the a-priori bound of an f32 sum of 128 terms in any
    order); nothing written past the last row / block.  The wrapper's total adds the blocks in
    f32: blocks - 1 more roundings."""
    nat = M["nat"]
    for rows in _rows_list(cols):
        gy, y = _relu_operands(rows, cols, 100 * cols + rows)
        want = torch.where(y > 0, gy, torch.zeros_like(gy))
        assert torch.equal(_bits(want), _bits(torch.ops.aten.threshold_backward(gy, y, 0.0)))
        blocks = -(-rows // 128)
        g, part = Guarded((rows + 3, cols), rows), Guarded((blocks + 2, cols), blocks)
        gyd, yd = gy.cuda(), y.cuda()
        nat.check(nat.lib().fjsp_a2c_relu_bias_grad(_ptr(gyd), _ptr(yd), rows, cols, _ptr(g.view), _ptr(part.view), _stream()))
        torch.cuda.synchronize()
        got, gp = g.check(), part.check()
        s, mag = _block_sums(want.double(), blocks)
        err = (gp.double() - s).abs()
        _report(kernel="relu_bias_grad", cols=cols, rows=rows, g_bits_differ=int((_bits(got) != _bits(want)).sum()),
                part_err_over_bound=float((err / (128 * U32 * mag).clamp_min(1e-300)).max()))
        assert torch.equal(_bits(got), _bits(want))
        assert bool((err <= 128 * U32 * mag).all())
        g2, total = A._relu_bias_grad(gyd, yd)
        assert torch.equal(_bits(g2.cpu()), _bits(want))
        assert bool(((total.cpu().double() - s.sum(0)).abs() <= (128 + blocks - 1) * U32 * mag.sum(0)).all())


def test_value_head_grad_edges(M):
    """g bit-equal to the f32 product gv w4 where y > 0, else +0; part[block] words [0, 128) against
    sum g, [128, 256) against sum gv y, [256] against sum gv, each within 129 u sum |terms| (128
    additions and the product's rounding) + 129 x 2^-149 (a product below the normal range rounds
    by up to 2^-150 whatever its size); [257, 260) exactly 0.  The row counts of both column
    widths' lists above (this kernel covers 8 rows a pass)."""
    nat = M["nat"]
    for rows in sorted(set(_rows_list(128)) | set(_rows_list(256))):
        _, y = _relu_operands(rows, 128, 7000 + rows)
        gen = torch.Generator().manual_seed(rows)
        gv = torch.randn(rows, generator=gen)
        if rows >= 3:
            gv[rows // 2] = 0.0                        # between the edge rows
        if rows >= 8:
            assert bool((gv > 0).any()) and bool((gv < 0).any())
        w4 = torch.randn(128, generator=gen)
        want = torch.where(y > 0, gv[:, None] * w4[None, :], torch.zeros_like(y))
        blocks = -(-rows // 128)
        g, part = Guarded((rows + 3, 128), rows), Guarded((blocks + 2, 260), blocks)
        yd, gvd, w4d = y.cuda(), gv.cuda(), w4.cuda()
        nat.check(nat.lib().fjsp_a2c_value_head_grad(_ptr(yd), _ptr(gvd), _ptr(w4d), rows, _ptr(g.view), _ptr(part.view),
                                                     _stream()))
        torch.cuda.synchronize()
        got, gp = g.check(), part.check()
        worst = 0.0
        sums = (("b3", 0, 128, want.double()), ("w4", 128, 256, gv.double()[:, None] * y.double()),
                ("b4", 256, 257, gv.double()[:, None]))
        fails = []
        for name, lo, hi, terms in sums:
            s, mag = _block_sums(terms, blocks)
            err, bound = (gp[:, lo:hi].double() - s).abs(), 129 * U32 * mag + 129 * UNDERFLOW
            worst = max(worst, float((err / bound).max()))
            if not bool((err <= bound).all()):
                fails.append(name)
        _report(kernel="value_head_grad", rows=rows, g_bits_differ=int((_bits(got) != _bits(want)).sum()),
                part_err_over_bound=worst)
        assert torch.equal(_bits(got), _bits(want))
        assert not fails, fails
        assert bool((_bits(gp[:, 257:260]) == 0).all())


def test_value_head_function_against_float64_autograd(M):
    """_ValueHead.apply at 129 rows (a full block and a block of one row; mlp_forward selects the
    Function only from 65 536 rows): its five gradients against float64 autograd of the same two
    layers, each entry within 129 u sum |terms| of its sum.  The layer's forward is exact in f32 by
    construction (small-integer h and W3, half-integer b3: every pre-activation a half-integer far
    below 2^24), so both sides share the ReLU mask and y, and the bound covers the backward alone."""
    g = torch.Generator().manual_seed(12)
    rows = 129
    h = torch.randint(0, 4, (rows, 256), generator=g).float()
    W3 = torch.randint(-2, 3, (128, 256), generator=g).float()
    b3 = torch.randint(-3, 3, (128,), generator=g).float() + 0.5
    W4, b4 = torch.randn(1, 128, generator=g), torch.randn(1, generator=g)
    wgt = torch.randn(rows, 1, generator=g)
    wgt[5] = 0.0
    leaves64 = [t.double().requires_grad_(True) for t in (h, W3, b3, W4, b4)]
    y64 = torch.relu(leaves64[0] @ leaves64[1].t() + leaves64[2])
    ((y64 @ leaves64[3].t() + leaves64[4]) * wgt.double()).sum().backward()
    assert 0.2 < float((y64 > 0).double().mean()) < 0.8
    leaves = [t.cuda().requires_grad_(True) for t in (h, W3, b3, W4, b4)]
    v = A._ValueHead.apply(*leaves)
    (v * wgt.cuda()).sum().backward()
    gv, y = wgt.double().reshape(-1), y64.detach()
    gabs = (gv[:, None] * W4.double()).abs() * (y > 0)                                   # |g| [rows, 128]
    mags = [gabs @ W3.double().abs(), gabs.t() @ h.double().abs(), gabs.sum(0), (gv.abs()[None] @ y.abs()),
            gv.abs().sum().reshape(1)]
    for name, leaf, l64, mag in zip(("h", "W3", "b3", "W4", "b4"), leaves, leaves64, mags):
        err = (leaf.grad.cpu().double() - l64.grad).abs()
        bound = 129 * U32 * mag.reshape(err.shape) + 129 * UNDERFLOW
        _report(kernel="_ValueHead", grad=name, err_over_bound=float((err / bound).max()))
        assert bool((err <= bound).all()), name


# ---------------------------------------------------------------- fjsp_a2c_critic_fused
FUSED_KEYS = ("h1", "h2", "g3", "g2", "g1", "values", "part", "loss")


def run_fused(M, kind, U, pad=True):
    """One direct fjsp_a2c_critic_fused call on critic_operands(kind, U) -> its outputs on the CPU
    after the sentinel checks (rows >= U, tiles >= ceil(U / 32) and the guards untouched); kept for
    the tests that compare launches."""
    key = (kind, U, pad)
    if key in M["fused"]:
        return M["fused"][key]
    nat = M["nat"]
    critic, x, coef = R.critic_operands(kind, U, pad)
    n = copy.deepcopy(critic).cuda().net
    with torch.no_grad():
        cw = A.pack_critic_weights(*[t for i in (0, 2, 4, 6) for t in (n[i].weight, n[i].bias)])
        w3t, w2t = A.pack_mfma(n[4].weight.t()).reshape(-1), A.pack_mfma(n[2].weight.t()).reshape(-1)
    xr = torch.nn.functional.pad(x.cuda(), (0, 2)).contiguous()
    tiles = -(-U // 32)
    rows = 32 * tiles + 4
    out = {k: Guarded((rows, 128 if k == "g3" else 256), U) for k in ("h1", "h2", "g3", "g2", "g1")}
    out["values"] = Guarded((rows,), U)
    out["part"] = Guarded((tiles + 2, R.PW), tiles)
    out["loss"] = Guarded((tiles + 2,), tiles, torch.float64)
    cd = coef.cuda()
    P = lambda k: _ptr(out[k].view)  # noqa: E731
    nat.check(nat.lib().fjsp_a2c_critic_fused(_ptr(xr), U, _ptr(cw), _ptr(w3t), _ptr(w2t), _ptr(cd), P("h1"), P("h2"), P("g3"),
                                              P("g2"), P("g1"), P("part"), P("loss"), P("values"), _stream()))
    torch.cuda.synchronize()
    res = {k: out[k].check() for k in FUSED_KEYS}
    res.update(critic=critic, x=x, coef=coef)
    M["fused"][key] = res
    return res


def fused_reference(res):
    """The masks of one launch (the kernel's m1, m2; m3 from g3 where gv w4 != 0, else float64's),
    the agreement of all three with float64 at the decided units, the float64 reference and the f32
    yardstick under those masks."""
    critic, x, coef = res["critic"], res["x"], res["coef"]
    share, d = R.critic_conditions(critic, x)                      # asserted here too, not re-derived
    z1, z2, z3, v64 = R.critic_forward64(critic, x)
    gv64 = coef[:, 0] * v64 + coef[:, 1]
    w4 = R.critic_params(critic)[6].reshape(1, -1)
    m1, m2 = res["h1"] > 0, res["h2"] > 0
    m3 = torch.where(gv64[:, None] * w4 != 0, res["g3"] != 0, z3 > 0)
    flips = []
    for m, z, dd in ((m1, z1, d[0]), (m2, z2, d[1]), (m3, z3, d[2])):
        assert bool((m == (z > 0))[dd].all())
        flips.append(int((m != (z > 0)).sum()))
    ref = R.critic_backward64(critic, x, coef, m1, m2, m3)
    yard = R.critic_backward32(critic, x, coef, m1, m2, m3)
    return ref, yard, share, flips


def _compare(rows, name, got, ref, yard, **tags):
    """One tensor under the rule kernel error <= 3 x yardstick error + 2^-23 max |ref| (max abs)."""
    ek = float((got.double() - ref).abs().max())
    ey = float((yard.cpu().double() - ref).abs().max())
    tol = 3 * ey + 2.0 ** -23 * float(ref.abs().max())
    rows.append(dict(tensor=name, err_kernel=ek, err_torch_f32=ey, tol=tol, ok=ek <= tol, **tags))


def _segments(part):
    return [("part." + n, part[:, lo:hi]) for n, lo, hi in R.PART_SEGMENTS]


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("U", R.CRITIC_U)
def test_critic_fused_outputs_match_float64(M, kind, U):
    """h1, h2, g3, g2, g1, the values, every word of every part[tile] (by segment: the b1, b2, b3,
    w4 and b4 sums) and loss[tile] against the float64 reference under the kernel's own masks; no
    state is excluded.  The masks agree with float64 at every decided unit; part[tile][769..771] is
    exactly 0; the padding state's gradient rows are exact zeros."""
    _check_fused(run_fused(M, kind, U), kind, U, R.padding_state(U))


@pytest.mark.parametrize("kind", ["init", "trained"])
def test_critic_fused_single_live_state(M, kind):
    """U = 1 once more with a live state (the list above has its padding state there, whose
    gradients are all zero): the same comparisons on a launch of one state with a gradient."""
    res = run_fused(M, kind, 1, pad=False)
    assert float(res["g3"].abs().max()) > 0 and float(res["g1"].abs().max()) > 0
    _check_fused(res, kind, 1, None)


def _check_fused(res, kind, U, pad_state):
    ref, yard, share, flips = fused_reference(res)
    rows = []
    for k in ("h1", "h2", "values", "g3", "g2", "g1", "loss"):
        _compare(rows, k, res[k], ref[k], yard[k], kind=kind, U=U)
    for (k, got), (_, want), (_, y) in zip(_segments(res["part"]), _segments(ref["part"]), _segments(yard["part"])):
        _compare(rows, k, got, want, y, kind=kind, U=U)
    for r in rows:
        _report(kernel="critic_fused", padded=pad_state is not None, undecided_share=share, flipped_units=flips, **r)
    assert all(r["ok"] for r in rows), [r for r in rows if not r["ok"]]
    assert bool((_bits(res["part"][:, 769:772]) == 0).all())
    if pad_state is not None:
        assert all(bool((res[k][pad_state] == 0).all()) for k in ("g1", "g2", "g3"))
    assert bool((res["h1"] >= 0).all()) and bool((res["h2"] >= 0).all())


@pytest.mark.parametrize("kind", ["init", "trained"])
def test_critic_fused_tiles_do_not_depend_on_the_launch(M, kind):
    """Bit for bit: states 0..31 (and tile 0's part / loss) of the U = 33, 64, 65 and 97 launches
    equal the U = 32 launch's; tile 1 of U = 65 and 97 equals tile 1 of U = 64."""
    for base, tile, others in ((32, 0, (33, 64, 65, 97)), (64, 1, (65, 97))):
        want = run_fused(M, kind, base)
        s = slice(32 * tile, 32 * tile + 32)
        for U in others:
            got = run_fused(M, kind, U)
            for k in ("h1", "h2", "g3", "g2", "g1", "values"):
                assert torch.equal(_bits(got[k][s]), _bits(want[k][s])), (U, k)
            for k in ("part", "loss"):
                assert torch.equal(_bits(got[k][tile]), _bits(want[k][tile])), (U, k)


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("U", [33, 97])
def test_critic_onepass_gradients_at_ragged_tiles(M, kind, U):
    """critic_onepass (the autograd Function: the kernel, the tile sums added, fjsp_a2c_wgrad) at
    one full tile + one state and at three tiles + one state: the loss and the eight parameter
    gradients against the float64 reference under the masks of the direct call on the same
    operands (the kernel is deterministic), under the element-wise rule above."""
    res = run_fused(M, kind, U)
    ref, yard, _, _ = fused_reference(res)
    critic, x, coef = res["critic"], res["x"], res["coef"]
    cd = copy.deepcopy(critic).cuda()
    xr = torch.nn.functional.pad(x.cuda(), (0, 2)).contiguous()
    loss = A.critic_onepass(cd, xr, coef.cuda())
    loss.backward()
    rows = []
    _compare(rows, "loss", loss.detach().cpu(), ref["loss"].sum(), yard["loss"].sum().float(), kind=kind, U=U)
    names = [k for k, _ in cd.named_parameters()]
    for name, p, g64, g32 in zip(names, cd.parameters(), R.param_grads(ref, x.double()),
                                 R.param_grads(yard, x.cuda().float())):
        assert p.grad.shape == g64.shape
        _compare(rows, name, p.grad.cpu(), g64, g32, kind=kind, U=U)
    for r in rows:
        _report(kernel="critic_onepass", **r)
    assert all(r["ok"] for r in rows), [r for r in rows if not r["ok"]]


# ---------------------------------------------------------------- fjsp_a2c_wgrad
WGRAD_SHAPES = [(256, 256, 256), (128, 256, 256), (256, 40, 38)]
WGRAD_MAX_U = 10000


def _wgrad_rows(P):
    return sorted(u for u in {1, 15, 16, 17, 31, 32, 33, 16 * P - 1, 16 * P, 16 * P + 1, 32 * P + 1} if 0 < u <= WGRAD_MAX_U)


def _wgrad_operands(m, nx, U):
    torch.manual_seed(5)
    g = torch.randn(U, m, device="cuda") * (torch.rand(U, m, device="cuda") > 0.5)
    if nx == 40:
        x = torch.nn.functional.pad(torch.rand(U, 38, device="cuda") * 30, (0, 2)).contiguous()
    else:
        x = torch.relu(torch.randn(U, nx, device="cuda"))
    return g, x


@pytest.mark.parametrize("P", [1, 3, 256])
@pytest.mark.parametrize("m,nx,nout", WGRAD_SHAPES)
def test_wgrad_at_its_split_edges(M, m, nx, nout, P):
    """critic_wgrad with `parts` = P workgroups where the split over 16-sample stages changes: one
    stage more or less than the workgroups (U = 16 P -+ 1), a second round starting (32 P + 1), one
    ragged stage, for the three layer shapes.  Relative Frobenius error within max(3 x the split-K
    f32 GEMM's, 2e-6) (test_wgrad_kernel_matches_float64's), every ROW of the output within the
    same factor of that row's float64 norm, both wgrad_waves settings bit-equal."""
    L = M["nat"].lib()
    gall, xall = _wgrad_operands(m, nx, max(_wgrad_rows(P)))
    for U in _wgrad_rows(P):
        g, x = gall[:U].contiguous(), xall[:U].contiguous()
        ref = g.double().t() @ x[:, :nout].double()
        gw = A.critic_wgrad(g, x, nout, parts=P)
        assert gw.shape == (m, nout)
        try:
            assert L.fjsp_set_option(None, b"wgrad_waves", 8) == 0
            gw8 = A.critic_wgrad(g, x, nout, parts=P)
        finally:
            assert L.fjsp_set_option(None, b"wgrad_waves", 16) == 0
        e = float((gw.double() - ref).norm() / ref.norm())
        et = float((A._splitk_wgrad(g, x[:, :nout]).double() - ref).norm() / ref.norm())
        bound = max(3 * et, 2e-6)
        rerr, rnorm = (gw.double() - ref).norm(dim=1), ref.norm(dim=1)
        worst = float((rerr / rnorm.clamp_min(1e-300)).max())
        _report(kernel="wgrad", m=m, nx=nx, P=P, U=U, err=e, err_splitk_f32=et, bound=bound, worst_row=worst,
                waves_bit_equal=bool(torch.equal(gw, gw8)))
        assert e <= bound, (U, e, et)
        assert bool((rerr <= bound * rnorm).all()), (U, worst, bound)
        assert torch.equal(_bits(gw), _bits(gw8)), U


@pytest.mark.parametrize("m,nx,nout", WGRAD_SHAPES)
def test_wgrad_zero_rows_change_nothing(M, m, nx, nout):
    """A ragged last stage whose extra row of g is exactly zero: U = 17 with row 16 zeroed equals
    U = 16 bit for bit, with one workgroup and with 256 (the stage then lands in a workgroup of its
    own, whose partial is zero), for both wgrad_waves settings."""
    L = M["nat"].lib()
    g, x = _wgrad_operands(m, nx, 17)
    g[16] = 0.0
    for P in (1, 256):
        for waves in (16, 8):
            try:
                assert L.fjsp_set_option(None, b"wgrad_waves", waves) == 0
                a = A.critic_wgrad(g, x, nout, parts=P)
                b = A.critic_wgrad(g[:16].contiguous(), x[:16].contiguous(), nout, parts=P)
            finally:
                assert L.fjsp_set_option(None, b"wgrad_waves", 16) == 0
            assert torch.equal(_bits(a), _bits(b)), (P, waves)
            assert float(b.abs().max()) > 0


# ---------------------------------------------------------------- the grouped update
def _gpu_update(name, monkeypatch, collide=False):
    actors, critic, batch, count, mean, std, ref = R.update_case(name)
    ad, cd = copy.deepcopy(actors).cuda(), copy.deepcopy(critic).cuda()
    made = []

    class Spy(A.UpdateBatch):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(A, "UpdateBatch", Spy)
    if collide:    # 4-bit grouping keys: different inputs collide, the grouping's check must catch it
        gk = A.group_keys
        monkeypatch.setattr(A, "group_keys", lambda f3, rows=None: gk(f3, rows) & 0xF)
    z = torch.zeros(8, device="cuda")
    al, cl = A.A2CLosses.compute(ad, cd, *[t.cuda() for t in batch], A.gather_index("cuda"), A.mask_index("cuda"), 0.01,
                                 z if mean is None else mean.cuda(), z if std is None else std.cuda(), count, dedup=True)
    (al.sum() + cl).backward()
    params = list(ad.named_parameters()) + list(cd.named_parameters())
    flat = A.flat_grads(ad, cd)                                      # before any clipping
    grads, o = [], 0
    for _, p in params:
        grads.append(flat[o:o + p.numel()].reshape(p.shape))
        o += p.numel()
    assert o == flat.numel() and len(made) == 1
    return made[0], al.tolist(), float(cl), grads, ref, [k for k, _ in params]


@pytest.mark.parametrize("name", list(R.UPDATE_BATCHES))
def test_grouped_update_matches_float64(M, monkeypatch, name):
    """keys -> grouping -> forward_reps -> one-pass critic -> loss head -> run sums -> wgrad on the
    GPU (A2CLosses.compute(dedup=True) + backward) against _reference_f64 with logp_old the
    reference's own (ratio 1: the A2C gradient): losses rtol 1e-4 / atol 1e-6, every parameter
    tensor's max error <= 1e-4 max |g64| (test_dense_loss_and_gradient_match_float64's bounds, which
    the f32 dense CPU update meets on these batches: tests/test_backward_ref_host.py).  The oracle
    batch, an oracle batch of 5 steps x 103 envs, and a single sample (count 1: no normalisation)."""
    batch, al, cl, grads, ref, names = _gpu_update(name, monkeypatch)
    assert batch.head_kernel and batch.coef is not None              # the path under test
    R.check_update(al, cl, grads, ref, names, report=lambda **kw: _report(kernel="update", batch=name, **kw))


def test_update_with_colliding_keys_falls_back_to_dense(M, monkeypatch):
    """4-bit grouping keys: the grouping's check fails, the update runs dense on the GPU and meets
    the same bounds."""
    batch, al, cl, grads, ref, names = _gpu_update("oracle_24x6", monkeypatch, collide=True)
    assert batch.ga is None and batch.gc is None and not batch.head_kernel and batch.coef is None
    R.check_update(al, cl, grads, ref, names, report=lambda **kw: _report(kernel="update", batch="collide", **kw))
