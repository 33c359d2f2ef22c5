"""The host side of K35's entry points under AddressSanitizer: tests/asan/sgm_checks.c, a stand-alone program with its own ``main``
linked against the host-only sanitizer build of the library (depthmodelhardening_amd.build.build_asan).  Every argument check of
dmh_sgm_plan and dmh_sgm_disparity, the plan's byte counts and chunk counts; nothing is launched and nothing is loaded into Python."""
import os
import subprocess


def test_sgm_host_side_under_address_sanitizer():
    from depthmodelhardening_amd.build import ASAN_LIB_PATH, build_asan
    driver = build_asan(driver_name="sgm_checks")
    assert os.path.exists(ASAN_LIB_PATH)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([driver], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "sgm_checks: ok" in r.stdout
