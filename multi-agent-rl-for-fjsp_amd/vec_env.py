"""FJSPVecEnv — N reference environments stepped in lockstep on one MI355X.

Device-resident tensors in, device-resident tensors out (zero copy through the C-ABI).
All layouts are field-major SoA with the env index fastest ([F, N]), the layout the
kernels write coalesced; ``.t()`` gives the [N, F] view a network consumes.
"""
import ctypes

import numpy as np
import torch

from . import _native as nat
from .slablog import LogSet, _ptr
from .spec import AGENTS

NI32, NI8, NF32, NMASK, NA, NFEAT = 20, 12, 6, 29, 8, 38
POLICIES = {"random": 0, "unmasked": 0, "masked": 1, "heuristic": 2}   # FJSP_ACTIONS_*
# the perturbed heuristic (fjsp_actions_eps): not a fjsp_step_many mode, so actions() / the per-row paths only
POLICIES["eps_heuristic"] = -1


def eps8_of(eps):
    """epsilon as fjsp_actions_eps takes it: round(eps * 256), an integer in 0..256."""
    e = int(round(float(eps) * 256))
    if not 0 <= e <= 256:
        raise ValueError(f"eps must be in [0, 1], got {eps!r}")
    return e


def _step_many_mode(policy):
    mode = POLICIES[policy]
    if mode < 0:
        raise ValueError(f"policy {policy!r} is not a fjsp_step_many mode: use actions() + step(), "
                         f"evaluate_schedule, solve or search")
    return mode


class SearchEnd:
    """End records of fjsp_search_rollout for N envs (device tensors; fjsp_search_end)."""

    def __init__(self, N, device):
        self.steps = torch.full((N,), -1, dtype=torch.int32, device=device)
        self.flags = torch.zeros(N, dtype=torch.uint8, device=device)
        self.orders_completed = torch.zeros(N, dtype=torch.int32, device=device)
        self.packaged = torch.zeros(N, dtype=torch.int32, device=device)
        self.sim_time = torch.zeros(N, dtype=torch.float64, device=device)

    def struct(self):
        return nat.fjsp_search_end(*[getattr(self, k).data_ptr() for k in nat.SEARCH_END_FIELDS])

    def numpy(self):
        return {k: getattr(self, k).cpu().numpy() for k in nat.SEARCH_END_FIELDS}


class Buffers:
    """Output tensors for T steps of N envs (T = 1 for step/reset)."""

    def __init__(self, T, N, device, infos=True, next_obs=False, feats=False, obs=True, held=False, pack=False):
        z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=device)  # noqa: E731
        # held: the held-tray words int32 [T, 3, N] (fjsp_step_held; not part of fjsp_out)
        self.held = z(T, 3, N, dt=torch.int32) if held else None
        # pack: the packaging stations' pack words int32 [T, 4, N] (fjsp_step_sched; not part of fjsp_out)
        self.pack = z(T, 4, N, dt=torch.int32) if pack else None
        # feats: a2c global-state features f32 [T, 38, N] of the post-auto-reset observation
        self.feats = z(T, NFEAT, N, dt=torch.float32) if feats else None
        if not obs:   # a2c-only outputs: features, post-reset masks, rewards, term, trunc
            self.obs_i32 = self.obs_i8 = self.obs_f32 = self.masks = None
            self.results = self.orders_completed = self.packaged = self.sim_time = None
            self.next_i32 = self.next_i8 = self.next_f32 = None
            self.next_masks = z(T, NMASK, N, dt=torch.int8)
            self.rewards = z(T, NA, N, dt=torch.float64)
            self.term = z(T, N, dt=torch.uint8)
            self.trunc = z(T, N, dt=torch.uint8)
            self.status = z(T, N, dt=torch.int32)
            return
        self.obs_i32 = z(T, NI32, N, dt=torch.int32)
        self.obs_i8 = z(T, NI8, N, dt=torch.int8)
        self.obs_f32 = z(T, NF32, N, dt=torch.float32)
        self.masks = z(T, NMASK, N, dt=torch.int8)
        self.rewards = z(T, NA, N, dt=torch.float64)
        self.term = z(T, N, dt=torch.uint8)
        self.trunc = z(T, N, dt=torch.uint8)
        self.status = z(T, N, dt=torch.int32)
        if infos:
            self.results = z(T, NA, N, dt=torch.int32)
            self.orders_completed = z(T, N, dt=torch.int32)
            self.packaged = z(T, N, dt=torch.int32)
            self.sim_time = z(T, N, dt=torch.float64)
        else:
            self.results = self.orders_completed = self.packaged = self.sim_time = None
        if next_obs:
            self.next_i32 = z(T, NI32, N, dt=torch.int32)
            self.next_i8 = z(T, NI8, N, dt=torch.int8)
            self.next_f32 = z(T, NF32, N, dt=torch.float32)
            self.next_masks = z(T, NMASK, N, dt=torch.int8)
        else:
            self.next_i32 = self.next_i8 = self.next_f32 = self.next_masks = None

    def struct(self):
        o = nat.fjsp_out()
        for k in nat.OUT_FIELDS:
            t = getattr(self, k, None)
            setattr(o, k, t.data_ptr() if t is not None else None)
        return o


class RowBuffers:
    """Row k of a [T, ...] Buffers as the T = 1 outputs of one step (views, no copies)."""

    def __init__(self, b, k):
        for f in nat.OUT_FIELDS:
            t = getattr(b, f, None)
            setattr(self, f, None if t is None else t[k:k + 1])
        self._struct = Buffers.struct(self)

    def struct(self):
        return self._struct


class FJSPVecEnv:
    """N independent FJSP environments (reference semantics per env) on one GPU.

    Env ``e`` has global id ``env_id_base + e``; its default MT19937 stream is
    ``np.random.seed(global id)`` and synthetic actions are keyed by the global id, so
    results do not depend on how envs are sharded over GPUs.
    """

    def __init__(self, num_envs, device=None, config=None, env_id_base=0, **cfg_over):
        if not torch.cuda.is_available():
            raise nat.FjspNativeError("FJSPVecEnv needs a GPU (HIP); no CPU fallback exists")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.num_envs = int(num_envs)
        self.env_id_base = int(env_id_base)
        c = config if config is not None else nat.default_config(**cfg_over)
        self.config = c
        L = nat.lib()
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            nat.check(L.fjsp_create(ctypes.byref(c), self.num_envs, self.device.index or 0,
                                    ctypes.c_void_p(stream), ctypes.byref(h)))
        self._h = h
        self._step_buf = None
        self._num_orders = 30
        self._pending_seeds = None
        if self.env_id_base:
            # default streams keyed by global id: env e starts from np.random.seed(env_id_base + e),
            # whichever call resets it first (reset(seed=None), a learner's reset, ...)
            nat.check(L.fjsp_set_option(h, b"env_id_base", self.env_id_base))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                nat.lib().fjsp_destroy(h)
            except Exception:
                pass
            self._h = None

    # ------------------------------------------------------------------ helpers
    def _sync_stream(self):
        nat.check(nat.lib().fjsp_set_stream(self._h, ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    @property
    def handle(self):
        return self._h

    def state_bytes_per_env(self):
        return int(nat.lib().fjsp_state_bytes(self._h))

    def seed(self, seeds):
        """np.random.seed(seeds[e]) for every env (applied at the next reset)."""
        self._pending_seeds = torch.as_tensor(seeds, device=self.device).to(torch.int64).bitwise_and(0xFFFFFFFF).to(torch.int32)

    # ------------------------------------------------------------------ API
    def reset(self, seeds=None, env_mask=None, num_orders=30, buffers=None):
        """FJSPSimulation.reset for the selected envs (FJSPSimulation.py:286-323)."""
        self._sync_stream()
        self._num_orders = int(num_orders)
        if seeds is None and getattr(self, "_pending_seeds", None) is not None:
            seeds = self._pending_seeds
        self._pending_seeds = None
        s = None
        if seeds is not None:
            s = torch.as_tensor(seeds, device=self.device)
            s = s.to(torch.int64).bitwise_and(0xFFFFFFFF).to(torch.int32).contiguous()
        m = None
        if env_mask is not None:
            m = torch.as_tensor(env_mask, device=self.device).to(torch.uint8).contiguous()
        b = buffers or Buffers(1, self.num_envs, self.device, infos=False)
        out = b.struct()
        nat.check(nat.lib().fjsp_reset(self._h, _ptr(s), _ptr(m), self._num_orders, ctypes.byref(out)))
        return b

    def put_orders(self, orders, counts=None, env_mask=None, append=False, buffers=None, check=True):
        """Orders from the caller instead of the MT19937 draw (fjsp_put_orders, include/fjsp.h).

        orders: [K, N] words (orders.encode; a tensor or anything np.asarray takes), counts [N] the
        rows each env uses (None: K).  append=False: a reset with these orders as the episode's
        table, the env's stream neither reseeded nor advanced; append=True: the orders arrive in
        the running episode (ids norders.., the back of the pickup queue).  An env whose rows hold
        an invalid word, whose count is outside 0..K or (append) would pass 64 orders is left as it
        was and counted.  check=True reads that count (one synchronisation), raises ValueError
        naming it if it is not 0 and returns the Buffers with the written envs' observation;
        check=False returns the device counter (int32 [1]) without synchronising."""
        self._sync_stream()
        w = orders if isinstance(orders, torch.Tensor) else torch.as_tensor(np.asarray(orders).astype(np.int64))
        w = w.to(device=self.device, dtype=torch.int64).bitwise_and(0xFFFFFFFF)
        w = torch.where(w >= 2**31, w - 2**32, w).to(torch.int32).contiguous()
        if w.dim() != 2 or w.shape[1] != self.num_envs or w.shape[0] > 64:
            raise ValueError(f"orders must be [K, {self.num_envs}] with K <= 64, got {tuple(w.shape)}")
        K = int(w.shape[0])
        c = None
        if counts is not None:
            c = torch.as_tensor(counts, device=self.device).to(torch.int32).contiguous()
            if tuple(c.shape) != (self.num_envs,):
                raise ValueError(f"counts must be [{self.num_envs}], got {tuple(c.shape)}")
        m = None
        if env_mask is not None:
            m = torch.as_tensor(env_mask, device=self.device).to(torch.uint8).contiguous()
            if tuple(m.shape) != (self.num_envs,):
                raise ValueError(f"env_mask must be [{self.num_envs}], got {tuple(m.shape)}")
        b = buffers or Buffers(1, self.num_envs, self.device, infos=False)
        out = b.struct()
        rejected =torch.zeros(1, dtype=torch.int32, device=self.device)
        nat.check(nat.lib().fjsp_put_orders(self._h, _ptr(w) if K else None, K, _ptr(c), _ptr(m), int(bool(append)),
                                            _ptr(rejected), ctypes.byref(out)))
        if not check:
            return rejected
        n = int(rejected.item())
        if n:
            raise ValueError(f"put_orders: {n} env(s) rejected (an invalid order word, a count outside 0..K or more "
                             f"than 64 orders); they are unchanged")
        return b

    def reset_orders(self, orders, counts=None, env_mask=None, buffers=None, check=True):
        """put_orders(append=False): FJSPSimulation.reset with the caller's orders."""
        return self.put_orders(orders, counts, env_mask, False, buffers, check)

    def add_orders(self, orders, counts=None, env_mask=None, buffers=None, check=True):
        """put_orders(append=True): FJSPSimulation.generate_order calls between two steps."""
        return self.put_orders(orders, counts, env_mask, True, buffers, check)

    def _open(self, seeds, num_orders, orders, counts):
        """The opening reset of the evaluation methods: reset(seeds, num_orders), or with the caller's
        orders reset(seeds, num_orders=0) when seeds are given (it seeds the streams and draws
        nothing) and reset_orders(orders, counts)."""
        if orders is None:
            if counts is not None:
                raise ValueError("counts needs orders")
            return self.reset(seeds=seeds, num_orders=num_orders)
        if seeds is not None or self._pending_seeds is not None:
            self.reset(seeds=seeds, num_orders=0)
        return self.reset_orders(orders, counts)

    def solve(self, books, samples, policy="masked", steps=None, action_seed=0, packaging=False, eps=0.15):
        """Best-of-`samples` schedules of caller-written order books: env i * samples + r is replica r
        of books[i] (orders.encode's order tuples), so num_envs must be len(books) * samples.  Every
        replica runs evaluate_schedule(orders=...) for `steps` vector steps (default
        max_episode_steps + 1: every first episode ends) under `policy`, whose action stream is keyed
        by the env id, and kpis.best_of picks each book's winner among the first episodes.  Returns
        best_of's dict plus "ops" (and "pack_ops" with packaging=True): the winners' first-episode
        records, as ScheduleLog.pop() / PackagingLog.pop() return them.  eps: policy "eps_heuristic"'s
        epsilon (actions)."""
        from . import kpis as K
        from . import orders as O
        from . import schedule as S
        books, samples = [list(b) for b in books], int(samples)
        if samples < 1 or self.num_envs != len(books) * samples:
            raise ValueError(f"solve needs num_envs == len(books) * samples, got {self.num_envs} envs for "
                             f"{len(books)} books x {samples} samples")
        words, counts = O.encode([b for b in books for _ in range(samples)])
        steps = int(self.config.max_episode_steps) + 1 if steps is None else int(steps)
        r = self.evaluate_schedule(policy=policy, steps=steps, action_seed=action_seed, packaging=packaging,
                                   orders=words, counts=counts, eps=eps)
        out = K.best_of(r["kpis"], samples, instances=len(books), env_id_base=self.env_id_base)
        win = out["best_env"] + self.env_id_base
        for name, as_dict in (("ops", S.records_dict), ("pack_ops", S.pack_records_dict)):
            if name in r:
                recs = r[name]["records"]
                keep = np.isin(recs["env_gid"], win) & (recs["episode_start"] == 0)
                out[name] = as_dict(recs[keep], r[name]["dropped"])
        return out

    def actions(self, policy="heuristic", action_seed=0, step=0, out=None, eps=0.15):
        """The actions rollout(policy=..., action_seed=..., step0=step) would draw for the current
        state at vector step `step` (fjsp_actions): uint8 [8, N], what step() takes.  policy
        "eps_heuristic" (fjsp_actions_eps): the heuristic, each agent with probability eps (in steps
        of 1/256) taking "masked"'s draw of the same (action_seed, env, step) instead."""
        self._sync_stream()
        if out is None:
            out = torch.empty(NA, self.num_envs, dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or not out.is_contiguous() or out.device != self.device or \
                tuple(out.shape) != (NA, self.num_envs):
            raise ValueError(f"out must be a contiguous uint8 [8, {self.num_envs}] tensor on the env's device")
        if POLICIES[policy] < 0:
            nat.check(nat.lib().fjsp_actions_eps(self._h, eps8_of(eps), int(action_seed) & (2**64 - 1), self.env_id_base,
                                                 int(step), _ptr(out)))
            return out
        nat.check(nat.lib().fjsp_actions(self._h, POLICIES[policy], int(action_seed) & (2**64 - 1), self.env_id_base,
                                         int(step), _ptr(out)))
        return out

    def search_rollout(self, K, eps=0.15, action_seed=0, step_base=0, t0=0, script=None, script_len=None, active=None,
                       trace=None, end=None):
        """fjsp_search_rollout: one launch that runs every active env from its current state until its
        episode ends (or K steps), without auto-reset.  Step k of env e takes script[k, :, e] while
        k < script_len[e] (script uint8 [L, 8, N]; script_len int32 [N], None: L) and after that the
        "eps_heuristic" actions of vector step step_base + t0 + k; the actions go to trace[k, :, e]
        (uint8 [K, 8, N]; rows past an env's stop are not written).  active: uint8 [N] (None: all);
        an inactive env is untouched.  Returns (trace, end): end a SearchEnd with steps (k + 1 at the
        stop, -1: not within K or inactive), flags (bit 0 terminated, bit 1 truncated) and the
        orders_completed / packaged / sim_time infos of the env's last executed step."""
        self._sync_stream()
        K, N = int(K), self.num_envs
        if trace is None:
            trace = torch.zeros(max(K, 0), NA, N, dtype=torch.uint8, device=self.device)
        elif trace.dtype != torch.uint8 or not trace.is_contiguous() or trace.device != self.device or \
                trace.dim() != 3 or trace.shape[0] < K or tuple(trace.shape[1:]) != (NA, N):
            raise ValueError(f"trace must be a contiguous uint8 [>= {K}, 8, {N}] tensor on the env's device")
        L = 0
        if script is not None:
            if script.dtype != torch.uint8 or not script.is_contiguous() or script.device != self.device or \
                    script.dim() != 3 or tuple(script.shape[1:]) != (NA, N):
                raise ValueError(f"script must be a contiguous uint8 [L, 8, {N}] tensor on the env's device")
            L = int(script.shape[0])
        elif script_len is not None:
            raise ValueError("script_len needs a script")
        if script_len is not None:
            script_len = torch.as_tensor(script_len, device=self.device).to(torch.int32).contiguous()
            if tuple(script_len.shape) != (N,):
                raise ValueError(f"script_len must be [{N}], got {tuple(script_len.shape)}")
        if active is not None:
            active = torch.as_tensor(active, device=self.device).to(torch.uint8).contiguous()
            if tuple(active.shape) != (N,):
                raise ValueError(f"active must be [{N}], got {tuple(active.shape)}")
        end = end or SearchEnd(N, self.device)
        es = end.struct()
        nat.check(nat.lib().fjsp_search_rollout(self._h, K, eps8_of(eps), int(action_seed) & (2**64 - 1), self.env_id_base,
                                                int(step_base), int(t0), _ptr(script), L, _ptr(script_len), _ptr(active),
                                                _ptr(trace), ctypes.byref(es)))
        return trace, end

    def search(self, books, width, stride=8, eps=0.15, action_seed=0, max_passes=None, packaging=False):
        """Rollout search over caller-written order books (search.search): a best-of-`width` first
        pass under the perturbed heuristic, then passes that commit the incumbent's next `stride`
        steps and run `width` lanes from there to the episode's end, keeping a strictly better run.
        num_envs must be len(books) * width; env i * width + r is replica r of books[i]."""
        from . import search as SR
        return SR.search(self, books, width, stride=stride, eps=eps, action_seed=action_seed, max_passes=max_passes,
                         packaging=packaging)

    def step(self, actions, agent_order=None, autoreset=True, buffers=None, held=None, pack=None):
        """One FJSPSimulation.step per env (FJSPSimulation.py:144-242).

        actions: uint8 tensor [8, N] (agent-major) on the env's device.  held: an int32 / uint32
        [3, N] tensor (or a [1, 3, N] slab row) that receives the step's held-tray words
        (fjsp_step_held, schedule.py); None: plain fjsp_step.  pack (needs held): an int32 / uint32
        [4, N] tensor that receives the packaging stations' pack words (fjsp_step_sched)."""
        if pack is not None and held is None:
            raise ValueError("pack needs held: fjsp_step_sched stores both")
        self._sync_stream()
        a = actions
        if a.dtype != torch.uint8 or not a.is_contiguous() or a.device != self.device:
            a = a.to(device=self.device, dtype=torch.uint8).contiguous()
        if tuple(a.shape) != (NA, self.num_envs):
            raise ValueError(f"actions must be [8, {self.num_envs}], got {tuple(a.shape)}")
        if buffers is None:
            if self._step_buf is None:
                self._step_buf = Buffers(1, self.num_envs, self.device, infos=True, next_obs=True)
            buffers = self._step_buf
        order = None
        if agent_order is not None:
            order = (ctypes.c_uint8 * 8)(*[int(x) for x in agent_order])
        out = buffers.struct()
        if held is not None:
            if held.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not held.is_contiguous() or \
                    held.device != self.device or held.numel() != 3 * self.num_envs:
                raise ValueError(f"held must be a contiguous int32 [3, {self.num_envs}] tensor on the env's device")
            if pack is not None:
                if pack.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not pack.is_contiguous() or \
                        pack.device != self.device or pack.numel() != 4 * self.num_envs:
                    raise ValueError(f"pack must be a contiguous int32 [4, {self.num_envs}] tensor on the env's device")
                nat.check(nat.lib().fjsp_step_sched(self._h, _ptr(a), order, int(bool(autoreset)), ctypes.byref(out),
                                                    _ptr(held), _ptr(pack)))
                return buffers
            nat.check(nat.lib().fjsp_step_held(self._h, _ptr(a), order, int(bool(autoreset)), ctypes.byref(out),
                                               _ptr(held)))
            return buffers
        nat.check(nat.lib().fjsp_step(self._h, _ptr(a), order, int(bool(autoreset)), ctypes.byref(out)))
        return buffers

    def server_start(self, actions, autoreset=True, buffers=None):
        """Start the step server (fjsp_server_start): a resident kernel that steps every env once
        per server_step() on a host doorbell, no launch or stream synchronisation per step.
        actions: u8 [8, N] the caller rewrites before every server_step (pinned host memory, or a
        device tensor whose writes are complete); outputs go to `buffers` (T = 1).  actions=None on
        a one-env handle: inline mode, each server_step(actions) hands its 8 action bytes over in
        the doorbell's cache line (fjsp_server_step_actions)."""
        if actions is None:
            if self.num_envs != 1:
                raise ValueError("inline actions (actions=None) need a one-env handle")
        else:
            if actions.dtype != torch.uint8 or not actions.is_contiguous() or tuple(actions.shape) != (NA, self.num_envs):
                raise ValueError(f"actions must be a contiguous uint8 [8, {self.num_envs}] tensor")
            if actions.device.type == "cpu" and not actions.is_pinned():
                raise ValueError("host actions must be in pinned memory (the kernel reads them in place)")
        self._srv_inline = actions is None
        self._sync_stream()
        b = buffers or Buffers(1, self.num_envs, self.device, infos=False)
        self._srv_keep = (actions, b, b.struct())          # the kernel reads / writes these every step
        nat.check(nat.lib().fjsp_server_start(self._h, _ptr(actions), int(bool(autoreset)),
                                              ctypes.byref(self._srv_keep[2])))
        return b

    def server_step(self, actions=None):
        """One step of every env on the running (or relaunched) step server; returns when the
        step's outputs are written.  Inline mode: actions = the env's 8 action codes."""
        if getattr(self, "_srv_inline", False):
            a = np.ascontiguousarray(actions, dtype=np.uint8).reshape(-1)
            if a.size != NA:
                raise ValueError("inline server_step takes the env's 8 action codes")
            nat.check(nat.lib().fjsp_server_step_actions(self._h, ctypes.c_void_p(a.ctypes.data)))
        else:
            nat.check(nat.lib().fjsp_server_step(self._h))

    def server_stop(self):
        nat.check(nat.lib().fjsp_server_stop(self._h))

    def rollout(self, K, action_seed=0, step0=0, masked=False, autoreset=True, buffers=None, infos=False,
                policy=None):
        """K fused steps with on-device actions; returns [K, F, N] trajectories.

        policy: "random" (uniform, action_space.sample()), "masked" (uniform over valid
        actions) or "heuristic" (MultiAgentA2C._get_heuristic_actions, a2c.py:390-537)."""
        self._sync_stream()
        mode = _step_many_mode(policy) if policy is not None else (1 if masked else 0)
        b = buffers or Buffers(K, self.num_envs, self.device, infos=infos)
        out = b.struct()
        nat.check(nat.lib().fjsp_step_many(self._h, int(K), int(action_seed) & (2**64 - 1), self.env_id_base,
                                           int(step0), mode, int(bool(autoreset)), ctypes.byref(out)))
        return b

    def evaluate(self, policy="heuristic", num_orders=5, max_steps=500, seeds=None, action_seed=0, orders=None,
                 counts=None):
        """MultiAgentA2C.test (a2c.py:539-645) for every env at once: each env runs from a reset
        until its episode ends (term or trunc: the reference's `while env.agents`) or max_steps.
        Returns the reference's test() dict with one entry per env: steps, orders_completed,
        products_packaged, rewards_by_agent [8, N] (each agent's rewards summed in step order,
        as episode_rewards) and total_reward (their sum in agent order, a2c.py:626).  orders / counts:
        the caller's order books in place of the draw (_open; total_orders is then each env's count)."""
        _step_many_mode(policy)
        self._open(seeds, num_orders, orders, counts)
        if orders is not None:
            num_orders = np.asarray(torch.as_tensor(counts).cpu()) if counts is not None else int(len(orders))
        b = self.rollout(int(max_steps), action_seed=action_seed, policy=policy, autoreset=False, infos=True)
        done = (b.term | b.trunc).cpu().numpy().astype(bool)                  # [T, N]
        T = done.shape[0]
        first = np.where(done.any(0), done.argmax(0) + 1, T)                  # steps run per env
        live = np.arange(T)[:, None] < first[None, :]
        rew = np.where(live[:, None, :], b.rewards.cpu().numpy(), 0.0)        # [T, 8, N]
        by_agent = np.cumsum(rew, axis=0)[-1] if T else np.zeros((NA, self.num_envs))   # sequential
        idx = np.maximum(first - 1, 0)
        cols = np.arange(self.num_envs)
        pick = lambda x: x.cpu().numpy()[idx, cols] if T else np.zeros(self.num_envs, np.int32)  # noqa: E731
        return {"steps": first, "orders_completed": pick(b.orders_completed),
                "products_packaged": pick(b.packaged), "total_orders": num_orders,
                "rewards_by_agent": by_agent, "total_reward": np.cumsum(by_agent, axis=0)[-1]}

    def evaluate_episodes(self, policy="heuristic", num_orders=5, steps=500, seeds=None, action_seed=0, chunk=256,
                          orders=None, counts=None):
        """Every finished episode of every env over `steps` vector steps from a reset, with
        auto-reset (an env starts its next episode at once; a2c.py:346-381): rollout(chunk, ...)
        into one reused Buffers, each followed by EpisodeLog.scan on the device.  Returns
        EpisodeLog.pop()'s dict of records (env, length, end_step, total, by_agent [8, n], ...).
        Only the records reach the host; no reward slab is copied."""
        return self._evaluate_logged(policy, num_orders, steps, seeds, action_seed, chunk, kpis=False, orders=orders,
                                     counts=counts)["episodes"]

    def evaluate_kpis(self, policy="heuristic", num_orders=5, steps=500, seeds=None, action_seed=0, chunk=256,
                      orders=None, counts=None):
        """evaluate_episodes with the shop-floor KPIs beside the returns: the same loop, each chunk
        scanned into an EpisodeLog and a kpis.KpiLog (fjsp_kpi_scan over the chunk's result words,
        the stations' int8 observations, the infos and sim_time).  Returns {"episodes":
        EpisodeLog.pop(), "kpis": KpiLog.pop()}; record k of each describes the same episode
        (kpis.kpi_summary derives makespan, flow times, utilisation, ... from "kpis").  Only the
        records reach the host."""
        return self._evaluate_logged(policy, num_orders, steps, seeds, action_seed, chunk, orders=orders, counts=counts)

    def evaluate_schedule(self, policy="heuristic", num_orders=5, steps=500, seeds=None, action_seed=0, chunk=256,
                          packaging=False, orders=None, counts=None, eps=0.15):
        """evaluate_kpis with the per-operation schedule beside it: from a reset, per vector step
        the policy's actions (fjsp_actions) and one fjsp_step_held into row k of a chunk slab, each
        chunk scanned into an EpisodeLog, a kpis.KpiLog and a schedule.ScheduleLog.  The states and
        outputs are rollout()'s with the same seeds.  Returns {"episodes", "kpis", "ops"}; an op's
        (env, episode_start) is an episode record's (env, end_step - length).  Only the records
        reach the host.  packaging=True: the steps go through fjsp_step_sched, whose pack words feed a
        schedule.PackagingLog with the same rows, and the result has "pack_ops" = its pop() (one
        record per tray run at a packaging station; schedule.check_packaging, schedule.arrivals).  eps:
        policy "eps_heuristic"'s epsilon (actions)."""
        return self._evaluate_logged(policy, num_orders, steps, seeds, action_seed, chunk, schedule=True,
                                     packaging=bool(packaging), orders=orders, counts=counts, eps=eps)

    def evaluate_script(self, actions, orders, counts=None, packaging=False, seeds=None, chunk=256):
        """evaluate_schedule with each row's actions taken from the caller's uint8 [T, 8, N] tensor
        instead of a policy: T vector steps from reset_orders(orders, counts) through fjsp_step_held
        (fjsp_step_sched with packaging=True), with auto-reset.  Returns {"episodes", "kpis", "ops"}
        (and "pack_ops")."""
        a = torch.as_tensor(actions)
        if a.dim() != 3 or tuple(a.shape[1:]) != (NA, self.num_envs):
            raise ValueError(f"actions must be [T, 8, {self.num_envs}], got {tuple(a.shape)}")
        a = a.to(device=self.device, dtype=torch.uint8).contiguous()
        if orders is None:
            raise ValueError("evaluate_script needs orders")
        return self._evaluate_logged(None, 0, int(a.shape[0]), seeds, 0, chunk, schedule=True, packaging=bool(packaging),
                                     orders=orders, counts=counts, script=a)

    def _evaluate_logged(self, policy, num_orders, steps, seeds, action_seed, chunk, kpis=True, schedule=False,
                         packaging=False, orders=None, counts=None, eps=0.15, script=None):
        """The loop behind evaluate_episodes / _kpis / _schedule: from a reset, chunks of rows into one
        reused Buffers, each scanned into a slablog.LogSet; returns its pop().  Two rollout paths,
        which launch different kernels: one fjsp_step_many per chunk, or with schedule per row the
        policy's actions (fjsp_actions) and one fjsp_step_held / fjsp_step_sched.  orders / counts: the
        caller's order books for the first episodes in place of the draw (_open); later episodes are
        drawn from the envs' streams with the envs' order counts.  script (schedule only): uint8
        [steps, 8, N] on the device, row k's actions in place of the policy's."""
        if not schedule:
            _step_many_mode(policy)
        steps, chunk = int(steps), max(1, min(int(chunk), int(steps)))
        self._open(seeds, num_orders, orders, counts)
        logs = LogSet(self, steps, kpis=kpis, schedule=schedule, packaging=packaging)
        b = Buffers(chunk, self.num_envs, self.device, infos=True, held=schedule, pack=packaging)
        slabs = {name: getattr(b, name) for name in LogSet.SLABS}
        if schedule:
            rows = [RowBuffers(b, k) for k in range(chunk)]
            act = torch.empty(NA, self.num_envs, dtype=torch.uint8, device=self.device)
        done = 0
        while done < steps:
            k = min(chunk, steps - done)
            if schedule:
                for j in range(k):
                    if script is not None:
                        act = script[done + j]
                    else:
                        self.actions(policy, action_seed=action_seed, step=done + j, out=act, eps=eps)
                    self.step(act, autoreset=True, buffers=rows[j], held=b.held[j], pack=b.pack[j] if packaging else None)
            else:
                self.rollout(k, action_seed=action_seed, step0=done, policy=policy, autoreset=True, buffers=b)
            logs.scan(slabs, k)
            done += k
        return logs.pop()

    def pack_a2c(self, feats=None, masks=None):
        """a2c features f32 [38, N] and masks int8 [29, N] of the current observations
        (MultiAgentA2C._get_global_state, a2c.py:153-166)."""
        self._sync_stream()
        if feats is None:
            feats = torch.empty(NFEAT, self.num_envs, dtype=torch.float32, device=self.device)
        if masks is None:
            masks = torch.empty(NMASK, self.num_envs, dtype=torch.int8, device=self.device)
        nat.check(nat.lib().fjsp_pack_a2c(self._h, _ptr(feats), _ptr(masks)))
        return feats, masks

    def snapshot(self, out=None):
        """Copy of every env's complete state (uint8 tensor; device unless `out` is given)."""
        self._sync_stream()
        nb = int(nat.lib().fjsp_snapshot_bytes(self._h))
        if out is None:
            out = torch.empty(nb, dtype=torch.uint8, device=self.device)
        if out.numel() * out.element_size() != nb:
            raise ValueError(f"snapshot needs {nb} bytes")
        nat.check(nat.lib().fjsp_snapshot(self._h, _ptr(out)))
        return out

    def restore(self, snap):
        self._sync_stream()
        nb = int(nat.lib().fjsp_snapshot_bytes(self._h))
        if snap.numel() * snap.element_size() != nb:
            raise ValueError(f"snapshot of {snap.numel() * snap.element_size()} bytes, handle needs {nb}")
        nat.check(nat.lib().fjsp_restore(self._h, _ptr(snap.contiguous())))

    def reward_weights(self):
        """The handle's reward weights as {fjsp_reward_weights field: value} (the defaults until
        set_reward_weights; they belong to the handle and are not part of a snapshot)."""
        w = getattr(self, "_weights", None)
        if w is None:
            w = nat.fjsp_reward_weights()
            nat.check(nat.lib().fjsp_default_reward_weights(ctypes.byref(w)))
            self._weights = w
        return {k: float(getattr(w, k)) for k in nat.REWARD_FIELDS}

    def set_reward_weights(self, weights=None, **names):
        """fjsp_set_reward_weights: `weights` = a fjsp_reward_weights, sixteen values in its field
        order or a {field: value} mapping (None: keep the current ones), then single fields by
        name (case-insensitive, so RewardModel's ORDER_COMPLETE_REWARD works too).  Applies from
        the next launch or server step.  Returns the new weights as reward_weights() does."""
        cur = self.reward_weights()
        if isinstance(weights, nat.fjsp_reward_weights):
            weights = {k: getattr(weights, k) for k in nat.REWARD_FIELDS}
        elif weights is not None and not hasattr(weights, "keys"):
            vals = [float(x) for x in weights]
            if len(vals) != len(nat.REWARD_FIELDS):
                raise ValueError(f"{len(nat.REWARD_FIELDS)} reward weights expected, got {len(vals)}")
            weights = dict(zip(nat.REWARD_FIELDS, vals))
        for src in (weights or {}, names):
            for k, v in src.items():
                if k.lower() not in cur:
                    raise ValueError(f"unknown reward weight {k!r}")
                cur[k.lower()] = float(v)
        w = nat.fjsp_reward_weights(*[cur[k] for k in nat.REWARD_FIELDS])
        self._sync_stream()
        nat.check(nat.lib().fjsp_set_reward_weights(self._h, ctypes.byref(w)))
        self._weights = w
        return self.reward_weights()

    def last_kernel(self):
        """Name of the kernel variant of the last step launch (e.g. "k_step_pipe<lds>")."""
        return nat.lib().fjsp_last_kernel(self._h).decode()

    def last_kernel_ms(self):
        ms = ctypes.c_float()
        nat.check(nat.lib().fjsp_last_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def read_env(self, e):
        v = nat.fjsp_env_view()
        nat.check(nat.lib().fjsp_read_env(self._h, int(e), ctypes.byref(v)))
        return v

    def mt_get(self, e):
        import numpy as np
        key = np.zeros(624, np.uint32)
        pos = ctypes.c_int32()
        nat.check(nat.lib().fjsp_mt_get(self._h, int(e), ctypes.c_void_p(key.ctypes.data), ctypes.byref(pos)))
        return key, pos.value

    def mt_set(self, e, key, pos):
        import numpy as np
        k = np.ascontiguousarray(key, dtype=np.uint32)
        nat.check(nat.lib().fjsp_mt_set(self._h, int(e), ctypes.c_void_p(k.ctypes.data), int(pos)))

    def sync(self):
        nat.check(nat.lib().fjsp_sync(self._h))

    def faults(self, clear=False):
        """The handle's fault word (fjsp_faults; synchronises): bit 0 = a bounded hand-off wait
        of a multi-wave step kernel gave up (its envs carry FJSP_STATUS_SPIN_TIMEOUT)."""
        w = ctypes.c_uint32()
        nat.check(nat.lib().fjsp_faults(self._h, ctypes.byref(w), int(bool(clear))))
        return w.value


def gae(rewards, values, done, boot, gamma, lamb, out_ret=None, out_adv=None):
    """Returns + GAE (transition_memory.py:83-105) on device tensors.

    rewards f64 [T, M], values f32 or f64 [T, M], done u8 [T, N], boot f64 [M]; columns m = a*N + e."""
    T, M = rewards.shape
    N = done.shape[1]
    ret = out_ret if out_ret is not None else torch.empty_like(rewards)
    adv = out_adv if out_adv is not None else torch.empty_like(rewards)
    r = rewards.contiguous(); v = values.contiguous(); d = done.to(torch.uint8).contiguous(); b = boot.contiguous()
    stream = torch.cuda.current_stream(rewards.device).cuda_stream
    fn = nat.lib().fjsp_gae_f64 if v.dtype == torch.float64 else nat.lib().fjsp_gae
    if v.dtype not in (torch.float32, torch.float64):
        raise TypeError("values must be float32 or float64")
    nat.check(fn(_ptr(r), _ptr(v), _ptr(d), _ptr(b), T, N, M, float(gamma), float(lamb),
                 _ptr(ret), _ptr(adv), ctypes.c_void_p(stream)))
    return ret, adv


def gae_shared(rewards, values, done, gamma, lamb, out_ret=None, out_adv=None):
    """gae() with one value per env shared by its agents (fjsp_gae_shared): rewards f64
    [T, A, N], values f32 [T + 1, N] (row T = the bootstrap value), done u8/bool [T, N] ->
    ret, adv f64 [T, A, N]."""
    T, A, N = rewards.shape
    if values.dtype != torch.float32 or tuple(values.shape) != (T + 1, N) or tuple(done.shape) != (T, N):
        raise ValueError("gae_shared: values f32 [T + 1, N] and done [T, N] expected")
    ret = out_ret if out_ret is not None else torch.empty_like(rewards)
    adv = out_adv if out_adv is not None else torch.empty_like(rewards)
    r = rewards.contiguous(); v = values.contiguous(); d = done.to(torch.uint8).contiguous()
    stream = torch.cuda.current_stream(rewards.device).cuda_stream
    nat.check(nat.lib().fjsp_gae_shared(_ptr(r), _ptr(v), _ptr(d), T, N, A, float(gamma), float(lamb),
                                        _ptr(ret), _ptr(adv), ctypes.c_void_p(stream)))
    return ret, adv


__all__ = ["FJSPVecEnv", "Buffers", "RowBuffers", "SearchEnd", "gae", "gae_shared", "AGENTS"]
