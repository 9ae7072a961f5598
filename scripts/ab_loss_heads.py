"""A/B of the three actor loss heads' C entries (fjsp_a2c_actor_head, fjsp_a2c_actor_head_ppo,
fjsp_a2c_record_head) between two builds of the library, byte for byte.

  FJSP_LIB=<library> python scripts/ab_loss_heads.py dump <out.npz>
      the entries on the inputs of tests/test_gpu_ppo.py::_head_inputs at (T, n) = (3, 70), (5, 103)
      and (1, 256): the A2C head, the PPO head in record mode and with a constructed logp_old, and
      the record head per agent on records derived from the same inputs; every grad, sums and
      logp_out (filled with NaN before the launch) goes to out.npz.
  python scripts/ab_loss_heads.py compare <a.npz> <b.npz>
      exact equality of every array's bytes; exit status 1 on a difference.
  FJSP_LIB=<library> python scripts/ab_loss_heads.py slab [reps]
      the three heads `reps` times (default 20) on a 256 x 4096 slab (for a kernel trace).
"""
import ctypes
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

SHAPES = [(3, 70), (5, 103), (1, 256)]
EPS_CLIP, COEF = 0.2, 0.01


def V(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def heads(torch, A, nat, inp, logp_old, T, n, out=None):
    """Every head once on inp = _head_inputs(T, n) and its constructed logp_old; the outputs into
    out (name -> array)."""
    S, pu, g = inp["S"], inp["pu"], inp["g"]
    B = -(-S // 256)
    L = nat.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    E = lambda *sh, dt=torch.float32: torch.full(sh, float("nan"), dtype=dt, device="cuda")  # noqa: E731
    slab = (V(pu), pu.shape[2], V(g.inv), T, n, V(inp["masks"]), V(inp["actions"]), V(inp["adv"]), V(inp["mean"]),
            V(inp["std"]))
    res = {}
    grad, sums = E(29, S), E(8, B, 2, dt=torch.float64)
    nat.check(L.fjsp_a2c_actor_head(*slab, 1.0 / S, COEF, V(grad), V(sums), st))
    res["a2c"] = (grad, sums)
    for name, old in (("ppo_record", None), ("ppo_ratio", logp_old)):
        grad, sums, lo = E(29, S), E(8, B, 4, dt=torch.float64), E(8, S)
        nat.check(L.fjsp_a2c_actor_head_ppo(*slab, V(old), V(lo), EPS_CLIP, 1.0 / S, COEF, V(grad), V(sums), st))
        res[name] = (grad, sums, lo)
    # records: one per sample, standing for 1..7 samples, w = that many times the normalised advantage
    bits = (inp["m"].to(torch.int32) << torch.arange(8, device="cuda", dtype=torch.int32)[None, :, None]).sum(1)
    info = (bits | (inp["acts"].to(torch.int32) << 8)).to(torch.int32).contiguous()
    cnt = (1 + torch.arange(S, device="cuda") % 7).to(torch.int32)
    wsum = (inp["adv_n"].double() * cnt).contiguous()
    for a, k in enumerate(A.N_ACTIONS):
        grad, sums = E(k, S), E(B, 2, dt=torch.float64)
        nat.check(L.fjsp_a2c_record_head(V(pu[a]), pu.shape[2], V(g.inv[a]), S, k, V(info[a]), V(wsum[a]), V(cnt),
                                         1.0 / S, COEF, V(grad), V(sums), st))
        res[f"record{a}"] = (grad, sums)
    torch.cuda.synchronize()
    if out is not None:
        for name, arrs in res.items():
            for kind, t in zip(("grad", "sums", "logp_out"), arrs):
                out[f"T{T}_n{n}_{name}_{kind}"] = t.cpu().numpy()


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different arrays"
    diff = [k for k in a.files if a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    unwritten = [k for k in a.files if np.isnan(a[k]).any() or np.isnan(b[k]).any()]
    print(json.dumps({"arrays": len(a.files), "bytes": int(sum(a[k].nbytes for k in a.files)), "different": diff,
                      "with_nan": unwritten}))
    return 1 if diff or unwritten else 0


def main():
    mode = sys.argv[1]
    if mode == "compare":
        return compare(sys.argv[2], sys.argv[3])
    import torch
    A = importlib.import_module("multi-agent-rl-for-fjsp_amd.a2c_vec")
    nat = importlib.import_module("multi-agent-rl-for-fjsp_amd._native")
    hi = importlib.import_module("tests.test_gpu_ppo")
    if mode == "dump":
        out = {}
        for T, n in SHAPES:
            inp = hi._head_inputs(A, T, n, 5 + T)
            heads(torch, A, nat, inp, hi._constructed_logp_old(A, inp)[0], T, n, out)
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        np.savez(sys.argv[2], **out)
        print(json.dumps({"library": nat.LIB_PATH, "arrays": len(out), "out": sys.argv[2]}))
    elif mode == "slab":
        inp = hi._head_inputs(A, 256, 4096, 7)
        logp_old = hi._constructed_logp_old(A, inp)[0]
        for _ in range(int(sys.argv[2]) if len(sys.argv) > 2 else 20):
            heads(torch, A, nat, inp, logp_old, 256, 4096)
    else:
        raise SystemExit(__doc__)
    return 0


if __name__ == "__main__":
    sys.exit(main())
