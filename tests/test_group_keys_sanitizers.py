"""AddressSanitizer + UndefinedBehaviorSanitizer over the host form of the arithmetic of msj_bucket_rows_device and
msj_group_keys_device (mojo_simdjson_amd/csrc/group_keys_math.h through tests/group_keys_math_host.cpp): one stand-alone
program with its own main, tests/cpp/group_keys_sanitize.cpp, built here with -fsanitize=address,undefined
-fno-sanitize-recover=all and run over hostile records and codes -- bits at every edge of int64 and of the doubles, types,
flags and codes from anywhere, widths up to 2^63 - 1, origins at both ends -- with R in {0, 1, 255, 256, 257}, every n_parts
from 1 to 8 and every array an allocation of exactly its size, against arithmetic of its own (__int128).  Nothing is loaded
into Python."""
import os
import subprocess

from tests import helpers
from tests.test_sanitizers import SAN


def test_group_keys_math_asan():
    out = os.path.join(helpers.ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "group_keys_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + [os.path.join(helpers.ROOT, "tests", "cpp", "group_keys_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "group_keys_sanitize ok" in r.stdout
