"""Sanitizer runs on the host code: the kernel's state machine compiled for the
host (tests/hostsim, csrc/fjsp_env.h) and the parity oracle (oracle/fjsp_oracle.c), built
together with AddressSanitizer + UndefinedBehaviorSanitizer (no recovery: the first report
aborts), step 256 envs x 400 steps side by side with random and masked-random actions and
auto-resets, plus a stress configuration, and must agree byte for byte.  GPU code is not
sanitized (no GPU ASan on this pool)."""
import os
import subprocess

import pytest

from tests import hostsim_build as HB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not HB.have_compilers(), reason="needs the host C and C++ compilers")
def test_hostsim_and_oracle_under_asan_ubsan(tmp_path):
    exe = HB.build_program(tmp_path, [HB.source("san_main.cpp"), os.path.join(REPO, "oracle", "fjsp_oracle.c")], sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "256", "400"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "OK" in r.stdout and "mismatches" in r.stdout
    print(r.stdout)
