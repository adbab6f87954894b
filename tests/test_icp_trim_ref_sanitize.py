"""CPU: the trimmed ICP's statement (tests/cpp/icp_trim_ref.cpp + csrc/lgr_icp_math.h) under AddressSanitizer + UndefinedBehaviorSanitizer,
as a stand-alone program with its own main (tests/cpp/icp_trim_ref_sanitize.cpp) built with -fsanitize=address,undefined
-fno-sanitize-recover; any report aborts.  Nothing sanitized is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_icp_trim_statement_under_asan_and_ubsan(tmp_path):
    exe = os.path.join(str(tmp_path), "icp_trim_ref_sanitize")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "lidar-global-registration_amd", "csrc"),
                           os.path.join(cpp, "icp_trim_ref_sanitize.cpp"), os.path.join(cpp, "icp_trim_ref.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="4")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "icp_trim_ref_sanitize: 600 runs, 0 failures" in out.stdout
