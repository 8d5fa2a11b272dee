"""Numbers with ONE feature -- the '.', the 'e', the exponent's sign or last digit, a byte that ends nothing, the first
significant digit, the one non-zero digit behind a tie -- at a chosen place of the device readers' walks
(csrc/numbers_kernel.hip): WindowRuns, the lane path's 64-byte window in LDS from the number's 16-byte line on, and WaveRuns,
the wave path's 64-byte steps over numbers of more than 1 024 characters.  A generator, no tests:
tests/test_number_phases.py pins it on the CPU and runs msj_number_values_device over it on the device.

A case is (group, kind, phase, text).  A Layout places cases in one buffer, blanks in front of each number so that its
first byte lands at a chosen residue of the buffer (the device buffer is 16-byte aligned), `behind` holds the bytes that lie
in the device tensor past the buffer's end.  Expected values are Python's (tests.test_number_math.expected), bit for bit.

Group A, lane window: start residue s = 0 .. 15 (mod 16) x window offset o = 62 .. 65 of the feature (character o - s of
  the number; 62 and 63 are the last bytes served from LDS, 64 and 65 the first from memory), 7 kinds, both signs.
Group B, end of the buffer, lane path: the number is the last token, len % 16 = 0 .. 15, it ends at len or one blank in
  front of it, its length is each of 1 .. 15, 17 .. 48 and 65 .. 90; '7' in every byte behind len.
Group C, wave path: feature 64 k + r bytes behind the start of the run the reader walks, r = 0 .. 63, 11 kinds (C_KINDS); the kinds
  again at r = 0 in total lengths 1 023 .. 1 026 (C-threshold), a long number at every buffer residue (C-start), a long
  number as the last token with len 0 .. 63 bytes behind the start of its last step (C-end).
Group D, the fallback list filled to its capacity - 1, capacity and capacity + 1.

A kind whose name ends in "0" is the twin of the case in front of it: the same text with '0' in the far digit's place.
"""
import functools
import random
from collections import namedtuple

from tests import test_number_math as tnm

Case = namedtuple("Case", "group kind phase text")
Layout = namedtuple("Layout", "data cases starts residues mod behind")

SPAN_CAP = 1024                  # tokens_kernel.hip: kSpanCap; a number of more characters is MSJ_SPAN_LONG
EXACT_DIGITS = 800               # number_math.h: kExactDigits
LONG_WAVES = 512                 # numbers_kernel.hip: num_long's grid, kListBlocks / 4 blocks of 4 waves
TIE16 = b"9007199254740993"      # 2^53 + 1: halfway between 2^53 and 2^53 + 2
TIE19 = b"4611686018427388416"   # 2^62 + 512: halfway between 2^62 and 2^62 + 1024, 19 digits
BEHIND = b"7" * 64               # what lies behind len in groups B and C-end
OFFSETS = (62, 63, 64, 65)
A_KINDS = ("dot", "e", "esign", "elast", "x", "firstnz", "tie")
C_KINDS = ("int_dot", "frac_e", "frac_end", "frac_x", "exp_nz", "exp_end", "firstnz", "tie_frac", "tie_int", "sticky", "mult64")
MULT64_FORMS = ("zero_frac", "zero_exp", "tie_tail", "int_run")
B_LENGTHS = tuple(range(1, 16)) + tuple(range(17, 49)) + tuple(range(65, 91))


def fallback_capacity(n):
    """numbers_kernel.hip: msj_number_fallback_capacity (the device test asserts it from the library)"""
    return n // 16 + 4096


def digits(n, seed):
    """n decimal digits, the first not 0"""
    r = random.Random(seed)
    return (r.choice("123456789") + "".join(r.choice("0123456789") for _ in range(n - 1))).encode() if n > 0 else b""


def zeros(n):
    assert n >= 0, n
    return b"0" * n


def is_long(text, start, length):
    """MSJ_SPAN_LONG of a number without a blank or structural byte inside: 1 025 characters and still no end"""
    return len(text) > SPAN_CAP and start + 1 + SPAN_CAP < length


def pairs(cases):
    """(case with the far digit, its twin without) for every twin"""
    return [(a, b) for a, b in zip(cases, cases[1:]) if b.kind == a.kind + "0"]


def layout(cases, residues, mod, behind=b""):
    """The cases as one JSON array: number k is token 1 + 2 k and starts at residues[k] modulo mod"""
    out, starts = bytearray(b"["), []
    for c, r in zip(cases, residues):
        out += b" " * ((r - len(out)) % mod)
        starts.append(len(out))
        out += c.text + b","
    out[-1:] = b"]"
    return Layout(bytes(out), tuple(cases), tuple(starts), tuple(residues), mod, behind)


def last_token_layout(case, length_residue, mod, blank):
    """[1, <number> with the number as the last token: it ends at len (blank = 0) or one blank in front of it, and
    len % mod = length_residue; BEHIND lies behind len"""
    tail = case.text + b" " * blank
    head = b"[1," + b" " * ((length_residue - 3 - len(tail)) % mod)
    data = head + tail
    assert len(data) % mod == length_residue
    return Layout(data, (case,), (len(head),), (len(head) % mod,), mod, BEHIND)


# ---- A: the lane window ---------------------------------------------------------------------------------------------------

def _a_texts(kind, c, neg, seed):
    """[(kind, text)] with the kind's feature at character c"""
    sign = b"-" if neg else b""
    m = c - neg   # characters between the sign and the feature
    if kind == "dot":
        return [(kind, sign + digits(m, seed) + b"." + digits(3, seed + 1))]
    if kind == "e":
        return [(kind, sign + digits(m, seed) + (b"E" if c & 1 else b"e") + b"-41")]
    if kind == "esign":
        return [(kind, sign + digits(m - 1, seed) + b"e" + es + b"17") for es in (b"+", b"-")]
    if kind == "elast":
        return [(kind, sign + digits(m - 3, seed) + b"e-2" + b"%d" % (1 + c % 9))]
    if kind == "x":   # behind an integer's digits, behind a fraction's
        return [(kind, sign + digits(m - 11, seed) + b"." + digits(10, seed + 1) + b"x" if neg else digits(m, seed) + b"x")]
    if kind == "firstnz":
        return [(kind, sign + b"0." + zeros(m - 2) + b"7" + b"31")]
    out = []   # tie: 2^53 + 1 as the issue has it (the exact path decides), then the 19-digit tie whose twin Eisel-Lemire decides
    for d, name in ((b"1", kind), (b"0", kind + "0")):
        out.append((name, sign + TIE16 + b"." + zeros(m - 17) + d))
    for d, name in ((b"1", kind), (b"0", kind + "0")):
        out.append((name, sign + TIE19 + b"." + zeros(m - 20) + d))
    for d, name in ((b"1", kind), (b"0", kind + "0")):
        out.append((name, sign + TIE19 + zeros(m - 19) + d + b"e-%d" % (m - 18)))
    return out


@functools.lru_cache(maxsize=None)
def group_a():
    """-> Layout (mod 16); phase = (s, o)"""
    cases, residues = [], []
    for s in range(16):
        for o in OFFSETS:
            for ki, kind in enumerate(A_KINDS):
                for neg in (0, 1):
                    for name, text in _a_texts(kind, o - s, neg, 1000 * s + 10 * o + ki):
                        cases.append(Case("A", name, (s, o), text))
                        residues.append(s)
    return layout(cases, residues, 16)


# ---- B: the end of the buffer, lane path ----------------------------------------------------------------------------------

def _b_text(n):
    """n characters whose value changes when a '7' is read behind them: an integer, or a float that ends in its exponent"""
    if n <= 18:
        return b"-" + digits(n - 1, n) if n & 1 == 0 else digits(n, n)
    tail = (b"e-3", b"e5", b"E+2")[n % 3]
    p = 1 + n % 5
    return digits(p, n) + b"." + digits(n - p - 1 - len(tail), n + 1) + tail


@functools.lru_cache(maxsize=None)
def group_b():
    """-> [Layout] of one call each; phase = (len % 16, length of the number, blanks in front of len).  Every length with
    both endings at two residues eight apart, which go round with the lengths: every residue meets every class of lengths"""
    out = []
    for i, n in enumerate(B_LENGTHS):
        for blank in (0, 1):
            for res in ((5 * i) % 16, (5 * i + 8) % 16):
                out.append(last_token_layout(Case("B", "blank" if blank else "end", (res, n, blank), _b_text(n)), res, 16, blank))
    return tuple(out)


# ---- C: the wave path -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def halfway_decimals():
    """64 exact halfway decimals of more than 19 and fewer than 800 significant digits that round down: (mantissa with a '.', exponent
    suffix, count of significant digits)"""
    out, texts = [], tnm._halfway_texts(random.Random(31), 240)
    for t, above in zip(texts[0::3], texts[1::3]):
        mant, _, exp = t.partition(b"e")
        n = len(mant.replace(b".", b"").lstrip(b"0"))
        # (the tie goes to the even neighbour: only where that is the lower one does a digit behind it change the result)
        if 19 < n < EXACT_DIGITS and len(mant) < 1100 and float(t) != float(above):
            out.append((mant, b"e" + exp if exp else b"", n))
    assert len(out) >= 64
    return tuple(out[:64])


def c_texts(kind, n, neg, seed, total=None, form=None):
    """[(kind, text)]: the kind's feature n bytes behind the start of the run that the reader walks.  total: the text's
    length, made up with characters away from that run (None: the fewest)."""
    sign = b"-" if neg else b""

    def build(make, least):
        """make(k): the text with k filling characters"""
        k = least if total is None else total - len(make(0))
        while total is not None and len(make(k)) > total:   # (an exponent that names k grew by a digit)
            k -= 1
        assert k >= least and total in (None, len(make(k))), (kind, n, total)
        return make(k)

    es = (b"-", b"+", b"")[n % 3]
    if kind == "int_dot":    # value about 10^5
        return [(kind, build(lambda k: sign + b"1" + zeros(n) + b"." + digits(k, seed) + b"e-%d" % (n - 5), 1))]
    if kind == "frac_e":
        return [(kind, build(lambda k: sign + b"3." + digits(n, seed) + b"e-" + zeros(k) + b"5", 0))]
    if kind == "frac_end":
        return [(kind, build(lambda k: sign + digits(k, seed + 1) + b"." + digits(n, seed), 1))]
    if kind == "frac_x":
        return [(kind, build(lambda k: sign + digits(k, seed + 1) + b"." + digits(n, seed) + b"x", 1))]
    if kind == "exp_nz":
        return [(kind, build(lambda k: sign + digits(k, seed) + b".5e" + es + zeros(n) + b"12", 1))]
    if kind == "exp_end":
        return [(kind, build(lambda k: sign + digits(k, seed) + b".5e" + es + zeros(n - 2) + b"12", 1))]
    if kind == "firstnz":    # value about 10^5
        return [(kind, build(lambda k: sign + b"0." + zeros(n) + b"7" + digits(k, seed) + b"e%d" % (n + 5), 2))]
    if kind == "tie_frac":
        return [(name, build(lambda k: sign + TIE19 + b"." + zeros(n) + d + zeros(k), 0)) for d, name in ((b"1", kind), (b"0", kind + "0"))]
    if kind == "tie_int":
        return [(name, build(lambda k: sign + TIE19 + zeros(n) + d + zeros(k) + b"e-%04d" % (n + 1 + k), 0))
                for d, name in ((b"1", kind), (b"0", kind + "0"))]
    if kind == "sticky":
        mant, exp, count = halfway_decimals()[form]
        return [(name, build(lambda k: sign + mant + zeros(EXACT_DIGITS - count) + zeros(n) + d + zeros(k) + exp, 0))
                for d, name in ((b"1", kind), (b"0", kind + "0"))]
    assert kind == "mult64" and n % 64 == 0
    if form == "zero_frac":
        return [(kind, build(lambda k: sign + b"0." + zeros(n) + b"e" + zeros(k) + b"5", 0))]
    if form == "zero_exp":
        return [(kind, build(lambda k: sign + digits(k, seed) + b".5e" + es + zeros(n), 1))]
    if form == "tie_tail":
        return [(kind, build(lambda k: sign + TIE19 + b"." + zeros(n) + b"e" + zeros(k) + b"0", 0))]
    return [(kind, build(lambda k: sign + b"1" + digits(n, seed) + b"." + digits(k, seed + 1) + b"e-%d" % n, 1))]   # int_run


def sticky_steps(form):
    """Whole steps in front of the sticky digit's step: as many as make the text longer than 1 024 characters, one at least"""
    mant, _, count = halfway_decimals()[form]
    return max(1, -(-(1090 - len(mant) - (EXACT_DIGITS - count)) // 64))


@functools.lru_cache(maxsize=None)
def group_c():
    """-> (first Layout, second Layout), mod 64.  The first holds the kinds without a twin at every r, and C-start: more
    long numbers than num_long has waves.  The second holds the pairs at every r, and C-threshold.  phase = r, or the total
    length for C-threshold."""
    first, second = ([], []), ([], [])
    for ki, kind in enumerate(C_KINDS):
        cases, residues = second if kind in ("tie_frac", "tie_int", "sticky") else first
        for r in range(64):
            steps = sticky_steps(r) if kind == "sticky" else 16 + r % 3
            form = r if kind == "sticky" else MULT64_FORMS[r % 4] if kind == "mult64" else None
            n = 64 * steps + (0 if kind == "mult64" else r)
            for name, text in c_texts(kind, n, r & 1, 100 * ki + r, form=form):
                cases.append(Case("C", name, r, text))
                residues.append(r if kind == "mult64" else (5 * r + 11 * ki) % 64)
    for r in range(64):
        first[0].append(Case("C-start", "start", r, (b"-" if r & 1 else b"") + b"3." + digits(1088 + (37 * r) % 64, 7000 + r) + b"e-7"))
        first[1].append(r)
    for ki, kind in enumerate(C_KINDS):
        short = next(i for i, h in enumerate(halfway_decimals()) if h[1])   # in exponent form: 801 characters to the sticky run
        for form in (MULT64_FORMS if kind == "mult64" else (short,) if kind == "sticky" else (None,)):
            for total in (SPAN_CAP - 1, SPAN_CAP, SPAN_CAP + 1, SPAN_CAP + 2):
                n = 64 * (3 if kind == "sticky" else 15)
                for name, text in c_texts(kind, n, total & 1, 9000 + ki, total=total, form=form):
                    second[0].append(Case("C-threshold", name, total, text))
                    second[1].append((7 * len(second[0])) % 64)
    return layout(first[0], first[1], 64), layout(second[0], second[1], 64)


@functools.lru_cache(maxsize=None)
def group_c_end():
    """-> [Layout] of one call each: a long number as the last token, unterminated, len = the start of the walked run +
    64 * 17 + m, m = 0 .. 63 = phase.  "exp": the exponent's run ends at len (a '7' read behind it changes the exponent);
    "tie": the zeros behind the 19-digit tie end at len (a '7' read behind them breaks the tie)"""
    out = []
    for m in range(64):
        sign = b"-" if m & 1 else b""
        for kind, text in (("exp", sign + b"1.5e-" + zeros(64 * 17 + m - 1) + b"5"), ("tie", sign + TIE19 + b"." + zeros(64 * 17 + m))):
            out.append(last_token_layout(Case("C-end", kind, m, text), (37 * m) % 64, 64, 0))
    return tuple(out)


# ---- D: the fallback list and the capacity ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def group_d():
    """-> {delta: (data, count of exact-path numbers, count of numbers)} for delta = -1, 0, 1: an array of numbers that
    need the exact path and as many '1' as make their count equal the fallback capacity of the array's n = 2 numbers + 1
    tokens, plus delta"""
    out = {}
    for delta in (-1, 0, 1):
        found = [(slow, fast) for fast in range(5, 40) for slow in range(4096, 6000)
                 if slow == fallback_capacity(2 * (slow + fast) + 1) + delta]
        slow, fast = found[0]
        texts = tnm.fallback_texts(random.Random(41 + delta), (slow + 2) // 3)[:slow]
        texts[1:1] = [b"1"] * (fast // 2)
        texts += [b"1"] * (fast - fast // 2)
        out[delta] = (b"[" + b",".join(texts) + b"]", slow, slow + fast)
    return out


@functools.lru_cache(maxsize=None)
def clipped():
    """-> (data, number index of a long number, of an exact-path number): both with records of every kind in front of
    them -- fast, long, exact-path, a syntax error -- and more behind"""
    fb = tnm.fallback_texts(random.Random(43), 2)
    long_ = [c.text for c in group_c()[1].cases[:2]]
    texts = [b"1", b"2.5", long_[0], fb[0], b"12x", b"-7", long_[1], b"3", fb[1], fb[2], b"4e400", fb[3], b"5", long_[0], b"6"]
    return b"[" + b", ".join(texts) + b"]", 6, 8
