"""AddressSanitizer + UndefinedBehaviorSanitizer over the host form of the arithmetic of msj_dictionary_order_device and
msj_rank_rows_device (mojo_simdjson_amd/csrc/dictionary_order_math.h through tests/dictionary_order_math_host.cpp): one
stand-alone program with its own main, tests/cpp/dictionary_order_sanitize.cpp, built here with
-fsanitize=address,undefined -fno-sanitize-recover=all and run on the word fetch at every phase, end and misalignment, on a
pinned corpus and on 4 000 rounds of hostile arrays -- offsets from anywhere, V around the room, both paths, short budgets
continued, CONTINUE over state from anywhere, codes from anywhere.  Every array at its exact size.  Nothing is loaded into
Python."""
import os
import subprocess

from tests import helpers
from tests.test_sanitizers import SAN


def test_dictionary_order_math_asan():
    out = os.path.join(helpers.ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "dictionary_order_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + [os.path.join(helpers.ROOT, "tests", "cpp", "dictionary_order_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "dictionary_order_sanitize ok" in r.stdout
