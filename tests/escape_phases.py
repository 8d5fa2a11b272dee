"""Long escaped string bodies with ONE escape (or one short group of escapes) at a chosen place: at every phase of the
64-byte steps of the waves' walks (csrc/wave_unescape.h: wave_unescape; csrc/validate_block.h: wave_body_bad), in front of
the closing quote with a partial last step, and around the 4 096-byte piece borders of a body that the grid walks.  A
generator, no tests: tests/test_escape_phases.py pins it on the CPU and runs every wave walk over it on the device.

A body is  b"x" * pad + ESCAPE + b"y" * tail,  always more than LANE_BODY raw bytes, so a wave walks it from its first
byte; a line is {"s":"<body>"} (tokens { "s" : "<body>" }: the body's string is token 3).  The phase of a case is pad % 64:
the lane of the step in which the escape's backslash stands.

Family "phase": every kind at every phase 0 .. 63 with pad = phase (the walk's first step: nothing carried in) and with
pad = 1088 + phase (step 17: carry, last6 / prev_starts and cover all carried), tail >= 70.
Family "end": every kind with the escape ending t = 0 .. 6 bytes in front of the closing quote and a raw length of
1 088 + m, m = 1 .. 12: the last step holds m bytes, and the escape straddles into it, ends it or lies in front of it (17
whole steps, not 16, so that the sibling of a 12-byte escape is still longer than LANE_BODY).

Which kinds are valid is Python's: json.loads takes every VALID kind; the serial walker (tests/test_validate_math.walk)
gives 0 for them and the string error for every INVALID one -- a lone surrogate half is an error here, though json.loads
passes it through.  Every invalid line has a sibling, the same pad and tail with \\u20ac in the escape's place, as its
neighbour in the mixed window.  tests/test_escape_phases.py::test_corpus_on_cpu pins all of this.
"""
import functools
import json
from collections import namedtuple

from tests import helpers
from tests import test_validate_math as tvm

LANE_BODY = 1024           # csrc/wave_unescape.h, csrc/validate_block.h: kLaneBody
WAVE_BODY = 1 << 20        # csrc/validate_block.h: kWaveBody
PIECE = 4096               # csrc/validate_block.h: kChunk
CARRIED = 1088             # 17 whole steps in front of the escape's step
STRING_TOKEN = 3           # { "s" : "<body>" }
PAIR = b"\\ud83d\\ude00"
SIBLING = b"\\u20ac"

VALID = [("n", b"\\n"), ("quote", b'\\"'), ("backslash", b"\\\\"), ("slash", b"\\/"), ("u0041", b"\\u0041"), ("u00e9", b"\\u00e9"),
         ("u20ac", b"\\u20ac"), ("pair", PAIR), ("five_n", b"\\" * 5 + b"n"), ("four_n", b"\\" * 4 + b"n"), ("u20ac_twice", b"\\u20ac\\u20ac"),
         ("pair_twice", PAIR + PAIR)]
INVALID = [("q", b"\\q"), ("u00g9", b"\\u00g9"), ("lone_high", b"\\ud83d"), ("lone_low", b"\\ude00"), ("high_bmp", b"\\ud83d\\u0041"),
           ("high_high", b"\\ud83d\\ud83d"), ("high_x_low", b"\\ud83dx\\ude00"), ("high_backslash_low", b"\\ud83d\\\\ude00")]
INVALID_AT_END = [("cut", b"\\u00e")]   # family "end", t = 0 only: the closing quote stands where the fourth digit belongs
ESCAPES = dict(VALID + INVALID + INVALID_AT_END)

Case = namedtuple("Case", "family kind valid phase pad tail line value verdict sibling")


def body_of(pad, escape, tail):
    return b"x" * pad + escape + b"y" * tail


def line_of(body):
    return b'{"s":"' + body + b'"}'


def _case(oracle, family, kind, valid, pad, tail, escape=None, sibling=False):
    line = line_of(body_of(pad, ESCAPES[kind] if escape is None else escape, tail))
    idx = tvm.stage1(oracle, line)
    assert idx is not None and len(idx) == 5, line[-40:]
    code, token = tvm.walk(line, idx.tolist())
    value = json.loads(line.decode("utf-8")) if valid else None
    return Case(family, kind, valid, pad % 64, pad, tail, line, value, (code, token), sibling)


def _with_sibling(oracle, family, kind, pad, tail):
    """An invalid case and, behind it, its valid sibling: the same pad and tail around \\u20ac"""
    return [_case(oracle, family, kind, False, pad, tail), _case(oracle, family, kind, True, pad, tail, escape=SIBLING, sibling=True)]


def phase_places():
    """(pad, tail) of family "phase": 128 places, both pads of every phase; the tail makes the body longer than LANE_BODY and
    lets the length of the last step vary"""
    for phase in range(64):
        yield phase, LANE_BODY + 70 + phase % 7
        yield CARRIED + phase, 70 + phase % 5


def end_places(escape):
    """(pad, tail) of family "end": 84 places, t = tail = 0 .. 6, raw length CARRIED + 1 .. 12"""
    for m in range(1, 13):
        for t in range(7):
            yield CARRIED + m - t - len(escape), t


@functools.lru_cache(maxsize=None)
def corpus():
    """-> (valid cases, mixed cases): the valid kinds; and every invalid case followed by its sibling"""
    oracle = helpers.load_oracle()
    valid, mixed = [], []
    for kind, escape in VALID:
        valid += [_case(oracle, "phase", kind, True, pad, tail) for pad, tail in phase_places()]
        valid += [_case(oracle, "end", kind, True, pad, tail) for pad, tail in end_places(escape)]
    for kind, escape in INVALID:
        for pad, tail in phase_places():
            mixed += _with_sibling(oracle, "phase", kind, pad, tail)
        for pad, tail in end_places(escape):
            mixed += _with_sibling(oracle, "end", kind, pad, tail)
    for kind, escape in INVALID_AT_END:
        for m in range(1, 13):
            mixed += _with_sibling(oracle, "end", kind, CARRIED + m - len(escape), 0)
    return valid, mixed


def one_document_subset():
    """The cases of the one-document calls: every kind at the phases 52 .. 63 and 0 .. 5 of the carried pad, and all of
    family "end" (siblings left out)"""
    valid, mixed = corpus()
    near = set(range(52, 64)) | set(range(6))
    return [c for c in valid + mixed if not c.sibling and (c.family == "end" or (c.pad >= CARRIED and c.phase in near))]


# ---- bodies that the grid walks in pieces --------------------------------------------------------------------------------

HUGE = WAVE_BODY + PIECE + 1          # 257 whole pieces and one byte: borders at PIECE * 1 .. 257 from the body's first byte
VALID_DELTAS = range(-12, 7)
INVALID_DELTAS = {"high_bmp": range(-11, 1), "lone_low": range(-11, 1), "q": (-5, -1, 0, 1, 5), "u00g9": (-5, -1, 0, 1, 5)}


def _planted(plants):
    body = bytearray(b"x" * HUGE)
    for at, escape in plants:
        assert body[at:at + len(escape)] == b"x" * len(escape) and at + len(escape) < HUGE
        body[at:at + len(escape)] = escape
    return bytes(body)


@functools.lru_cache(maxsize=None)
def huge_valid():
    """-> (line, places): ONE body of HUGE bytes with every valid kind starting delta bytes from a piece border, delta in
    -12 .. +6, each (kind, delta) at a border of its own; places: (kind, delta, border, offset in the body)"""
    places, border = [], 1
    for kind, escape in VALID:
        for delta in VALID_DELTAS:
            places.append((kind, delta, border, border * PIECE + delta))
            border += 1
    assert border - 1 <= HUGE // PIECE
    return line_of(_planted([(at, ESCAPES[kind]) for kind, _, _, at in places])), places


@functools.lru_cache(maxsize=None)
def huge_invalid():
    """-> [(kind, delta, border, one_document, line)]: 34 bodies of HUGE bytes with one bad escape each, delta bytes from a
    piece border; the borders are spread over the body, the first and the last whole piece among them.  one_document: the
    body goes through the one-document call, else into the window.  The kinds alternate out of step, so that each call
    gets every delta of the two 12-long ranges from one of the two surrogate kinds: the one-document call \\ud83d\\u0041 at
    the odd deltas -11 .. -1 and the lone low surrogate at the even ones -10 .. 0, the window call the other halves;
    delta = -6 (the second six bytes start on the border) and delta = 0 reach both calls"""
    out = []
    for n, (kind, deltas) in enumerate(INVALID_DELTAS.items()):
        for i, delta in enumerate(deltas):
            border = (1, 256)[len(out)] if len(out) < 2 else 1 + (len(out) * 37) % 255
            out.append((kind, delta, border, (i + n) % 2 == 0, line_of(_planted([(border * PIECE + delta, ESCAPES[kind])]))))
    return out
