"""The C-ABI library loads on CPU and exports every symbol include/fjsp.h declares
(no compute calls: there is no GPU in the build container)."""
import ctypes
import os
import re

import pytest

from tests import gpu_util as G


def _declared():
    hdr = open(os.path.join(G.REPO, "include", "fjsp.h")).read()
    return sorted(set(re.findall(r"^\w[\w\s\*]*?\b(fjsp_\w+)\s*\(", hdr, re.M)))


def test_header_matches_binding_list():
    assert _declared() == sorted(G.native.EXPORTS)


def test_library_exports_every_symbol():
    L = G.native.lib()
    for name in _declared():
        assert hasattr(L, name), name
    assert L.fjsp_abi_version() == G.native.ABI_VERSION == 14
    for gone in ("forward", "backward"):   # ABI 14: the grouped critic's three-kernel entries left
        with pytest.raises(AttributeError):
            getattr(L, "fjsp_a2c_critic_" + gone)


def test_config_validation_without_gpu():
    nat = G.native
    c = nat.default_config()
    assert (c.num_trays, c.tray_capacity, c.step_size, c.max_episode_steps, c.pt_small, c.pt_big,
            c.pt_packaging, c.packaging_capacity) == (1000, 5, 10, 200, 60, 120, 30, 20)
    assert nat.lib().fjsp_check_config(ctypes.byref(c)) == 0
    bad = nat.default_config(pt_small=65)
    assert nat.lib().fjsp_check_config(ctypes.byref(bad)) != 0
    assert b"multiple of step_size" in nat.lib().fjsp_last_error()
    bad = nat.default_config(step_size=8)
    assert nat.lib().fjsp_check_config(ctypes.byref(bad)) != 0


def test_kernels_compiled_for_gfx950():
    data = open(G.native.LIB_PATH, "rb").read()
    assert b"gfx950" in data
    assert b"k_step_many" in data or b"_Z" in data


def test_a2c_layout_matches_spec():
    """fjsp_out.feats column order == spec.a2c_feature_index (pinned against the reference's
    _get_global_state by test_oracle_golden.py::test_oracle_heuristic_and_global_state)."""
    out = (ctypes.c_int32 * 38)()
    assert G.native.lib().fjsp_a2c_layout(out) == 0
    spec = __import__("importlib").import_module("multi-agent-rl-for-fjsp_amd.spec")
    assert list(out) == spec.a2c_feature_index()


def test_grouping_entries_validate_arguments_without_gpu():
    """The grouping / run-sum entries (ABI 8) reject bad shapes and null buffers before touching
    the device: too many rows (the row id has 4 key bits), sizes past 32-bit positions, null
    buffers, an empty run-sum batch."""
    L = G.native.lib()
    P = ctypes.c_void_p
    one = P(1)
    cnt = ctypes.c_uint64()
    assert L.fjsp_a2c_group_temp_bytes(0, ctypes.byref(cnt)) != 0
    assert L.fjsp_a2c_group_temp_bytes(1 << 31, ctypes.byref(cnt)) != 0
    assert L.fjsp_a2c_group_sort(one, 17, 100, 0, one, 1 << 20, one, one, one, one, one, one, one, None) != 0
    assert b"R <= 16" in L.fjsp_last_error()
    assert L.fjsp_a2c_group_sort(one, 9, 1 << 28, 0, one, 1 << 20, one, one, one, one, one, one, one, None) != 0
    assert L.fjsp_a2c_group_sort(None, 9, 100, 0, one, 1 << 20, one, one, one, one, one, one, one, None) != 0
    assert b"null" in L.fjsp_last_error()
    assert L.fjsp_a2c_group_runs(one, one, 9, 100, 0, one, one, one, one, one, one, one, None) != 0
    assert L.fjsp_a2c_run_sums_bytes(0, 100, ctypes.byref(cnt)) != 0
    assert L.fjsp_a2c_run_sums_bytes(29, 100, ctypes.byref(cnt)) == 0 and cnt.value > 0
    assert L.fjsp_a2c_run_sums(one, 29, one, None, one, one, 100, 8, one, 0, one, None) != 0
    assert b"temp buffer too small" in L.fjsp_last_error()
    assert L.fjsp_a2c_run_sums(one, 70000, one, None, one, one, 100, 8, one, 1 << 30, one, None) != 0


def test_critic_fused_validates_arguments_without_gpu():
    """fjsp_a2c_critic_fused (ABI 9) rejects an empty batch, null buffers and unaligned rows before
    launching."""
    L = G.native.lib()
    P = ctypes.c_void_p
    a = P(1 << 20)
    args = [a, 64, a, a, a, a, a, a, a, a, a, a, a, None, None]
    bad = list(args)
    bad[1] = 0
    assert L.fjsp_a2c_critic_fused(*bad) != 0 and b"n must be > 0" in L.fjsp_last_error()
    bad = list(args)
    bad[5] = None
    assert L.fjsp_a2c_critic_fused(*bad) != 0 and b"null" in L.fjsp_last_error()
    bad = list(args)
    bad[0] = P((1 << 20) + 4)
    assert L.fjsp_a2c_critic_fused(*bad) != 0 and b"16-byte aligned" in L.fjsp_last_error()


def test_update_kernels_validate_arguments_without_gpu():
    """The ABI-9 update entries (record head, weight packing, slab statistics, combiner keys)
    reject bad shapes and null buffers before launching."""
    L = G.native.lib()
    P = ctypes.c_void_p
    a = P(1 << 20)
    assert L.fjsp_a2c_record_head(a, 8, a, 0, 3, a, a, a, 1.0, 0.01, a, a, None) != 0
    assert L.fjsp_a2c_record_head(a, 8, a, 10, 9, a, a, a, 1.0, 0.01, a, a, None) != 0
    assert L.fjsp_a2c_record_head(a, 8, None, 10, 3, a, a, a, 1.0, 0.01, a, a, None) != 0
    assert L.fjsp_a2c_pack_mfma(a, 1, 48, 16, 0, a, None) != 0 and b"multiple of 32" in L.fjsp_last_error()
    assert L.fjsp_a2c_pack_mfma(a, 1, 64, 20, 0, a, None) != 0
    assert L.fjsp_a2c_pack_mfma(a, 1, 64, 16, 0, P((1 << 20) + 4), None) != 0
    assert L.fjsp_a2c_slab_stats(None, None, 4, 4, a, a, a, None) != 0
    assert L.fjsp_a2c_slab_stats(a, None, 4, 4, None, a, None, None) != 0
    assert L.fjsp_a2c_slab_stats(a, a, 0, 4, a, a, a, None) != 0
    assert L.fjsp_a2c_shard_keys(a, a, a, 0, 4, a, a, a, None) != 0
    assert L.fjsp_a2c_shard_keys(a, None, a, 4, 4, a, a, a, None) != 0


def test_wgrad_validates_arguments_without_gpu():
    """fjsp_a2c_wgrad (ABI 12) rejects empty batches, null buffers, unaligned or ragged rows and
    unsupported layer shapes before launching."""
    L = G.native.lib()
    P = ctypes.c_void_p
    a = P(1 << 20)
    ok = [a, 256, 256, a, 256, 256, 1000, a, 256, a, 256, 256, None]

    def bad(i, v, msg):
        b = list(ok)
        b[i] = v
        assert L.fjsp_a2c_wgrad(*b) != 0 and msg in L.fjsp_last_error(), (i, v)
    bad(6, 0, b"must be > 0")
    bad(8, 0, b"must be > 0")
    bad(3, None, b"null")
    bad(9, None, b"null")
    bad(0, P((1 << 20) + 4), b"16-byte aligned")
    bad(4, 38, b"16-byte aligned")            # nx % 4 != 0
    bad(2, 128, b"16-byte aligned")           # ldg < m
    bad(10, 300, b"nout")
    bad(1, 64, b"(m, nx)")
    assert L.fjsp_set_option(None, b"wgrad_waves", 12) != 0
    assert L.fjsp_set_option(None, b"wgrad_waves", 8) == 0 and L.fjsp_set_option(None, b"wgrad_waves", 16) == 0


def test_library_wide_policy_options_without_gpu():
    """ABI 10: the policy launches' variants are library-wide options (fjsp_set_option with a null
    handle), validated; nothing else is settable without a handle, and nothing is read from the
    process environment."""
    L = G.native.lib()
    for name, v in ((b"policy_xmap", 2), (b"policy_xmap", 0), (b"policy_dedup", 0), (b"policy_dedup", 1),
                    (b"policy_split", 0), (b"policy_split", 1)):
        assert L.fjsp_set_option(None, name, v) == 0, name
    assert L.fjsp_set_option(None, b"policy_xmap", 4) != 0
    assert L.fjsp_set_option(None, b"policy_bogus", 1) != 0
    assert L.fjsp_set_option(None, b"pipeline", 1) != 0 and b"null handle" in L.fjsp_last_error()
    data = open(G.native.LIB_PATH, "rb").read()
    for var in (b"FJSP_POLICY_XMAP", b"FJSP_FUSED_LDS", b"FJSP_AGENTS", b"FJSP_PREDRAW"):
        assert var not in data, var
