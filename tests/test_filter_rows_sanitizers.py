"""AddressSanitizer + UndefinedBehaviorSanitizer over the host form of the arithmetic of msj_predicates_create,
msj_filter_rows_device and msj_take_rows_device (mojo_simdjson_amd/csrc/filter_rows_math.h through
tests/filter_rows_math_host.cpp): one stand-alone program with its own main, tests/cpp/filter_rows_sanitize.cpp, built here
with -fsanitize=address,undefined -fno-sanitize-recover=all and run on the pinned numbers and strings of
tests/test_filter_rows_math.py and on 300 damaged inputs -- records with bits, types, flags and codes from a generator, list
offsets that descend or exceed R, take indices at R - 1, R and 0xFFFFFFFF and repeated, a row count below and above the
capacities, each capacity one short, the mask-only form.  Every array at its exact size.  Nothing is loaded into Python."""
import os
import subprocess

from tests import helpers
from tests.test_sanitizers import SAN


def test_filter_rows_math_asan():
    out = os.path.join(helpers.ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "filter_rows_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + [os.path.join(helpers.ROOT, "tests", "cpp", "filter_rows_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "filter_rows_sanitize ok" in r.stdout
