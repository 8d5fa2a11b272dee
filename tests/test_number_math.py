"""CPU check of the number conversion of msj_number_values_device (mojo_simdjson_amd/csrc/number_math.h).

The header is compiled for the host with g++ (tests/number_math_host.cpp), the way test_lane_math.py checks lane_math.h,
and compared with Python: the grammar as a regular expression, then int() / float() with the int64 and finite-range
rules, bit patterns compared (so -0.0 and 0.0 differ).  The table of 5^q significands is recomputed with Python integers.
The kernels that run this code on the device are covered by tests/test_numbers.py (-m gpu).
"""
import ctypes
import os
import random
import re
import struct
import subprocess
from decimal import Decimal, getcontext

import numpy as np
import pytest

from tests import helpers

BUILD = os.path.join(helpers.ROOT, "tests", "_build")
GRAMMAR = re.compile(rb"-?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?")
FOLLOW = set(b",:[]{} \t\n\r")
INT64, DOUBLE, ERR_SYNTAX, ERR_RANGE = 1, 2, 3, 4


def expected(text, pos=0):
    """(kind, bits) of the number at text[pos] (bytes past the end read as blanks)."""
    m = GRAMMAR.match(text, pos)
    if m is None or (m.end() < len(text) and text[m.end()] not in FOLLOW):
        return ERR_SYNTAX, 0
    s = m.group(0)
    if m.group(2) is None and m.group(3) is None:
        if len(s.lstrip(b"-")) > 20:
            return ERR_RANGE, 0  # (int() refuses texts this long)
        v = int(s)
        if not -(1 << 63) <= v < (1 << 63):
            return ERR_RANGE, 0
        return INT64, v & ((1 << 64) - 1)
    f = float(s)
    if f in (float("inf"), float("-inf")):
        return ERR_RANGE, 0
    return DOUBLE, struct.unpack("<Q", struct.pack("<d", f))[0]


@pytest.fixture(scope="module")
def nm():
    return load_twin()


def load_twin():
    """The host twin (g++ build of tests/number_math_host.cpp), also what tests/test_numbers.py compares the GPU with."""
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libnumber_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "number_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.nm_convert.restype = ctypes.c_uint32
    lib.nm_convert.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                               ctypes.POINTER(ctypes.c_uint32)]
    lib.nm_convert_batch.restype = None
    lib.nm_convert_batch.argtypes = [ctypes.c_char_p, ctypes.c_uint64] + [ctypes.c_void_p] * 5
    lib.nm_convert_batch.argtypes[3] = ctypes.c_uint64
    lib.nm_pow5.argtypes = [ctypes.c_int32, ctypes.c_void_p]
    lib.nm_floor_log2_pow5.restype = ctypes.c_int32
    lib.nm_floor_log2_pow5.argtypes = [ctypes.c_int32]
    return lib


def convert_all(nm, texts, sep=b","):
    """The twin on every text, as one buffer joined by `sep`: -> (kinds, bits, path counts)."""
    buf = sep.join(texts)
    lens = np.fromiter((len(t) + len(sep) for t in texts), dtype=np.uint64, count=len(texts))
    starts = np.zeros(len(texts), dtype=np.uint64)
    starts[1:] = np.cumsum(lens)[:-1]
    bits = np.zeros(len(texts), dtype=np.uint64)
    kinds = np.zeros(len(texts), dtype=np.uint32)
    paths = np.zeros(3, dtype=np.uint64)
    nm.nm_convert_batch(buf, len(buf), starts.ctypes.data, len(texts), bits.ctypes.data, kinds.ctypes.data, paths.ctypes.data)
    return kinds, bits, paths


def fallback_texts(rng, count):
    """Numbers every one of which takes the exact path: decimal halfway points (2m + 1) * 2^(k - 1) between adjacent
    doubles written as (2m + 1) * 5^j followed by e-j, with more than 19 digits, and the same one unit above and below."""
    out = []
    for _ in range(count):
        m = rng.randrange(1 << 52, 1 << 53)
        j = rng.randrange(5, 40)
        k = rng.randrange(-30, 1)  # (k > 0 would give trailing zeros: an exact tie Eisel-Lemire decides)
        n = (2 * m + 1) * 5 ** j  # (2m + 1) * 2^-j = n * 10^-j; times 2^k below
        e = -j
        n = n << k if k >= 0 else n * 5 ** -k
        e = e if k >= 0 else e + k
        out += [f"{n}e{e}".encode(), f"{n + 1}e{e}".encode(), f"{n - 1}e{e}".encode()]
    return out


def check(nm, texts, sep=b","):
    kinds, bits, paths = convert_all(nm, texts, sep)
    for t, k, b in zip(texts, kinds.tolist(), bits.tolist()):
        want = expected(t + sep)
        assert (k, b) == want, (t[:80], len(t), (k, hex(b)), (want[0], hex(want[1])))
    return paths


def pow5_entry(q):
    if q >= 0:
        p = 5 ** q
        L = p.bit_length() - 1
        sh = 127 - L
        return p << sh if sh >= 0 else p >> -sh
    L = -((5 ** -q).bit_length())
    return (1 << (127 - L)) // 5 ** -q + 1


def test_pow5_table(nm):
    out = (ctypes.c_uint64 * 2)()
    for q in range(-342, 309):
        t = pow5_entry(q)
        nm.nm_pow5(q, out)
        assert (out[0] << 64 | out[1]) == t, q
        assert (1 << 127) <= t < (1 << 128)
        exact_l = (5 ** q).bit_length() - 1 if q >= 0 else -((5 ** -q).bit_length())
        assert nm.nm_floor_log2_pow5(q) == exact_l, q


def _halfway_texts(rng, count):
    """Exact decimal halfway points between adjacent doubles (normals and subnormals), and the same with one more digit
    above or below: from Decimal at 1 200 digits."""
    getcontext().prec = 1200
    out = []
    for _ in range(count):
        if rng.random() < 0.2:
            bits = rng.randrange(1, 1 << 52)  # subnormal
        else:
            bits = rng.randrange(1 << 52, 0x7FEFFFFFFFFFFFFF)
        lo = struct.unpack("<d", struct.pack("<Q", bits))[0]
        hi = struct.unpack("<d", struct.pack("<Q", bits + 1))[0]
        h = (Decimal(lo) + Decimal(hi)) / 2  # exact: both are dyadic, 1 200 digits hold the sum
        s = format(h, "f") if rng.random() < 0.3 else format(h, "e")
        mant, _, exp = s.partition("e")
        mant = mant if "." in mant else mant + ".0"
        base = mant + ("e" + exp if exp else "")
        out.append(base.encode())
        out.append((mant + "1" + ("e" + exp if exp else "")).encode())  # above
        # below: the same value minus one unit in a new last place
        d = Decimal(mant) - Decimal(1).scaleb(-(len(mant.split(".")[1]) + 1))
        out.append((format(d, "f") + ("e" + exp if exp else "")).encode())
    return out


def test_random_doubles(nm):
    """10^6 random doubles, each as repr, %.17e, %.25e and %.40g."""
    rng = np.random.default_rng(11)
    raw = rng.integers(0, 0x7FF0000000000000, 1_000_000, dtype=np.uint64, endpoint=False)
    raw |= (rng.integers(0, 2, raw.size, dtype=np.uint64) << np.uint64(63))
    vals = raw.view(np.float64)
    texts = []
    for v in vals.tolist():
        texts += [repr(v).encode(), b"%.17e" % v, b"%.25e" % v, b"%.40g" % v]
    kinds, bits, paths = convert_all(nm, texts)
    want_bits = np.repeat(raw, 4)
    # %.40g of an integral double prints no '.' and no exponent: those are integers (checked one by one below)
    is_float = np.array([(b"." in t or b"e" in t) for t in texts])
    assert (kinds[is_float] == DOUBLE).all()
    bad = np.nonzero(is_float & (bits != want_bits))[0]
    assert bad.size == 0, [texts[i] for i in bad[:5]]
    for i in np.nonzero(~is_float)[0].tolist():
        assert (int(kinds[i]), int(bits[i])) == expected(texts[i]), texts[i]
    print("random doubles: paths fast / lemire / exact =", paths.tolist())


def test_integers(nm):
    rng = random.Random(5)
    texts = [str(rng.randrange(-(1 << 63), 1 << 63)).encode() for _ in range(200_000)]
    for c in (1 << 53, 1 << 63, -(1 << 63), 10 ** 19, -(10 ** 19), 10 ** 18, 0):
        texts += [str(c + d).encode() for d in (-1, 0, 1)]
    texts += [b"0", b"-0", b"9223372036854775807", b"-9223372036854775808", b"9223372036854775808",
              b"-9223372036854775809", b"99999999999999999999", b"12345678901234567890", b"1" + b"0" * 40]
    # as floats too, around 2^53 and 2^63
    for c in (1 << 53, 1 << 63, 1 << 64):
        texts += [f"{c + d}.0".encode() for d in range(-3, 4)] + [f"{c + d}e0".encode() for d in range(-3, 4)]
    check(nm, texts)


def test_halfway_points(nm):
    paths = check(nm, _halfway_texts(random.Random(7), 1500))
    print("halfway points: paths fast / lemire / exact =", paths.tolist())
    assert paths[2] > 0


def test_fallback_corpus_takes_the_exact_path(nm):
    texts = fallback_texts(random.Random(9), 3000)
    paths = check(nm, texts)
    assert paths.tolist() == [0, 0, len(texts)]


def boundary_texts():
    """The boundary values, long and strange inputs."""
    texts = [b"4.9406564584124654e-324", b"2.4703282292062327e-324", b"2.4703282292062328e-324", b"2.4703282292062326e-324",
             b"2.2250738585072011e-308", b"2.2250738585072014e-308", b"2.2250738585072012e-308", b"2.2250738585072013e-308",
             b"1.7976931348623157e308", b"1.7976931348623158e308", b"1.7976931348623159e308", b"-1.7976931348623159e308",
             b"1e400", b"-1e400", b"1e-400", b"-1e-400", b"-0.0", b"0.0", b"-0e5", b"0e-5", b"1e308", b"1e-323", b"1e-324",
             b"2.4703282292062327208828439643411068618252990130716238221279284125033775363510437593264991818081799618989828234772285886546332835517796989819938739800539093906315035659515570226392290858392449105184435931802849936536152500319370457678249219365623669863658480757001585769269903706311928279558551332927834338409351978015531246597263579574622766465272827220056374006485499977096599470454020828166226237857393450736339007967761930577506740176324673600968951340535537458516661134223766678604162159680461914467291840300530057530849048765391711386591646239524912623653881879636239373280423891018672348497668235089863388587925628302755995657524455507255189313690836254779186948667994968324049705821028513185451396213837722826145437693412532098591327667236328125e-324",
             b"2.4703282292062327208828439643411068618252990130716238221279284125033775363510437593264991818081799618989828234772285886546332835517796989819938739800539093906315035659515570226392290858392449105184435931802849936536152500319370457678249219365623669863658480757001585769269903706311928279558551332927834338409351978015531246597263579574622766465272827220056374006485499977096599470454020828166226237857393450736339007967761930577506740176324673600968951340535537458516661134223766678604162159680461914467291840300530057530849048765391711386591646239524912623653881879636239373280423891018672348497668235089863388587925628302755995657524455507255189313690836254779186948667994968324049705821028513185451396213837722826145437693412532098591327667236328125001e-324",
             b"0." + b"0" * 400 + b"1e400", b"1e0000000000000000000001", b"0e99999999999999999999",
             b"1e-99999999999999999999", b"1e99999999999999999999", b"-1e-99999999999999999999", b"123.456e-0000000000000000000000000000000000000002",
             b"9007199254740993", b"9007199254740993.0", b"90071992547409930e-1", b"9007199254740992.5", b"0.1", b"0.3",
             b"1e23", b"8.98846567431158e307", b"1.0000000000000002", b"1.00000000000000011102230246251565404236316680908203125",
             b"1.00000000000000011102230246251565404236316680908203124", b"1.00000000000000011102230246251565404236316680908203126",
             b"7.2057594037927933e16", b"179769313486231580793728971405303415079934132710037826936173778980444968292764750946649017977587207096330286416692887910946555547851940402630657488671505820681908902000708383676273854845817711531764475730270069855571366959622842914819860834936475292719074168444365510704342711559699508093042880177904174497791.9999999999"]
    # mantissas of 800, 10 000 and 100 000 digits
    rng = random.Random(3)
    for n in (800, 10_000, 100_000):
        d = "".join(rng.choice("0123456789") for _ in range(n))
        texts += [("1" + d).encode(), ("0." + d).encode(), ("1." + d + "e-" + str(n)).encode(), ("-9." + d + "e-330").encode(),
                  ("2.4703282292062327208828439643411068618252990130716238221279284125033775363510437593264991818081799618989828234"
                   + "0" * n + "1e-324").encode(),
                  ("2.4703282292062327208828439643411068618252990130716238221279284125033775363510437593264991818081799618989828234772285886546332835517796989819938739800539093906315035659515570226392290858392449105184435931802849936536152500319370457678249219365623669863658480757001585769269903706311928279558551332927834338409351978015531246597263579574622766465272827220056374006485499977096599470454020828166226237857393450736339007967761930577506740176324673600968951340535537458516661134223766678604162159680461914467291840300530057530849048765391711386591646239524912623653881879636239373280423891018672348497668235089863388587925628302755995657524455507255189313690836254779186948667994968324049705821028513185451396213837722826145437693412532098591327667236328125"
                   + "0" * n + "1e-324").encode()]
    return texts


def test_boundaries_and_strange_inputs(nm):
    paths = check(nm, boundary_texts())
    print("boundaries: paths fast / lemire / exact =", paths.tolist())


SYNTAX = [b"01", b"-", b"1.", b"1.e5", b"1e", b"1e+", b"1.5x", b'1.5"b"', b"12a", b"-01", b"+1", b".5", b"1..2", b"1e5e5",
          b"--1", b"0x10", b"1.5e", b"-.5", b"00", b"1e-", b"Infinity", b"NaN", b"-a"]


def test_syntax(nm):
    texts = SYNTAX
    kinds, _, _ = convert_all(nm, texts, sep=b" ")
    assert kinds.tolist() == [ERR_SYNTAX] * len(texts)
    # the bad string of test_tokens.test_spans_follow_the_reference_scans, token by token (a number starts at - or a digit)
    bad = b'[12a,-,--1,1+2,1.5x,1e5,-0.5E-3,0x10,1.,12 ,3\t,4\n,5:6,7"a",1.5"b" ,9]'
    starts = [i for i in range(len(bad)) if bad[i] in b"-0123456789" and (i == 0 or bad[i - 1] in b"[,: \t\n")]
    for s in starts:
        b, k = ctypes.c_uint64(), ctypes.c_uint32()
        nm.nm_convert(bad, len(bad), s, ctypes.byref(b), ctypes.byref(k))
        assert (k.value, b.value) == expected(bad[s:]), bad[s:s + 8]
    # bytes past the end read as blanks
    b, k = ctypes.c_uint64(), ctypes.c_uint32()
    nm.nm_convert(b"[1.25", 5, 1, ctypes.byref(b), ctypes.byref(k))
    assert (k.value, b.value) == expected(b"1.25")
    nm.nm_convert(b"[1.25x", 5, 1, ctypes.byref(b), ctypes.byref(k))
    assert (k.value, b.value) == expected(b"1.25")
