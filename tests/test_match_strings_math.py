"""CPU check of the arithmetic of msj_patterns_create and msj_match_strings_device
(mojo_simdjson_amd/csrc/match_strings_math.h).

The host twin (tests/match_strings_math_host.cpp: the header's fold, tiles, masked word, four-byte fetch, piece test, row
look-up, accept rule and cursor, the call built serially from them in the kernels' steps -- tiles, halo, passes) runs over
hand-made columns.  The yardsticks are the definition of include/msj_stage1.h written in Python twice and know nothing of the
header: ``re`` (the pieces escaped and joined by a lazy ``.*?``) and the brute-force minimum over all position sequences.
Every output is compared over its WHOLE array, each at its exact size and pre-filled, so a write at or past R shows.
``Column``, ``py_match``, ``expected`` and ``run_twin`` are also what the GPU tests use (tests/test_match_strings.py, -m gpu);
arrays from anywhere are tests/test_match_strings_sanitizers.py's.
"""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests import helpers
from tests import test_validate_math as tvm

MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
AT_START, AT_END, NOCASE = 1, 2, 4
NO_SUCH_FIELD = 20
ALPHABET = (0x00, ord("a"), ord("A"), ord("b"), 0x7F, 0x80, 0xFF)
PIECE_LENGTHS = (1, 2, 3, 4, 5, 8, 15, 16, 17, 255)


class MatchResult(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_values", ctypes.c_uint64),
                ("n_matched", ctypes.c_uint64), ("max_pieces", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


class SelectResult(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_documents", ctypes.c_uint64), ("n_paths", ctypes.c_uint64),
                ("n_found", ctypes.c_uint64), ("n_no_bits", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


FIELD = np.dtype([("bits", "<u8"), ("token", "<u4"), ("type", "u1"), ("flags", "u1"), ("code", "<u2")])

_twin = None


def load_twin():
    """The host twin of the call (g++ build of tests/match_strings_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libmatch_strings_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "match_strings_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32
    for name, args, res in (("msm_fold1", [u32], u32), ("msm_fold4", [u32], u32), ("msm_fetch4", [u32, u32, u32], u32),
                            ("msm_phase", [vp], u32), ("msm_load_word16", [vp, u64, u64, vp], None),
                            ("msm_upper_bound", [vp, u64, u64, u64], u64), ("msm_constants", [vp], None),
                            ("msm_compile", [vp, vp, u32, u32, vp], i32),
                            ("msm_match_strings", [i32, vp, vp, u32, vp, vp, u64, vp, vp, u64, vp, u64, vp, vp, u32, u32], i32)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    _twin = lib
    return lib


@pytest.fixture(scope="module")
def tw():
    return load_twin()


def constants(tw):
    out = np.zeros(8, dtype=np.uint32)
    tw.msm_constants(out.ctypes.data)
    return dict(zip(("threads", "run", "tile", "halo", "chunk", "stage", "byte_blocks", "row_blocks"), (int(x) for x in out)))


def ptr(a):
    return None if a is None else a.ctypes.data


# ---- patterns -----------------------------------------------------------------------------------------------------------------

def norm(spec):
    """bytes -> contains; (pieces, flags) as it is -> ([bytes], flags)"""
    if isinstance(spec, (bytes, bytearray)):
        return [bytes(spec)], 0
    return [bytes(x) for x in spec[0]], int(spec[1])


def flat(specs):
    """The twin's form of a list of patterns: uint32[n][6] (n_pieces, flags, four lengths) and the bytes back to back"""
    desc = np.zeros((max(len(specs), 1), 6), dtype=np.uint32)
    data = bytearray()
    for i, s in enumerate(specs):
        pieces, flags = norm(s)
        desc[i, 0], desc[i, 1] = len(pieces), flags
        for j, x in enumerate(pieces[:4]):
            desc[i, 2 + j] = len(x)
        data += b"".join(pieces)
    return desc, np.frombuffer(bytes(data) + b"\0", dtype=np.uint8).copy()


# ---- the definition, twice ----------------------------------------------------------------------------------------------------

def lower(b):
    return bytes(c + 32 if 65 <= c <= 90 else c for c in b)


def py_match(v, spec):
    """The place of the first match of ``spec`` in the value ``v``, or None: the definition through ``re``"""
    pieces, flags = norm(spec)
    if flags & NOCASE:
        v, pieces = lower(v), [lower(x) for x in pieces]
    rx = re.compile((rb"\A" if flags & AT_START else b"") + b".*?".join(map(re.escape, pieces)) + (rb"\Z" if flags & AT_END else b""), re.DOTALL)
    m = rx.search(v)
    return None if m is None else m.start()


def brute_match(v, spec):
    """The same as the minimum p_0 over ALL position sequences"""
    pieces, flags = norm(spec)
    if flags & NOCASE:
        v, pieces = lower(v), [lower(x) for x in pieces]
    n = len(pieces)

    def chains(j, at):
        """can pieces j.. be placed at or behind `at`"""
        s = pieces[j]
        for p in range(at, len(v) - len(s) + 1):
            if v[p:p + len(s)] != s:
                continue
            if j == n - 1:
                if not (flags & AT_END) or p + len(s) == len(v):
                    return True
            elif chains(j + 1, p + len(s)):
                return True
        return False

    s0 = pieces[0]
    for p0 in range(0, len(v) - len(s0) + 1):
        if (flags & AT_START) and p0 != 0:
            break
        if v[p0:p0 + len(s0)] != s0:
            continue
        if n == 1:
            if not (flags & AT_END) or p0 + len(s0) == len(v):
                return p0
        elif chains(1, p0 + len(s0)):
            return p0
    return None


# ---- a column from a list of rows ---------------------------------------------------------------------------------------------

class Column:
    """(offsets, valid, bytes) of ``rows``: bytes is a value; None a null row of no bytes; ("null", bytes) a null row whose
    bytes stand in the byte array all the same.  ``lead`` / ``tail``: bytes in front of the first row and behind the last that
    belong to no row.  ``extra``: live-looking offsets and valid bytes behind R.  ``residue``: the address of bytes[0] mod 16."""

    def __init__(self, rows, lead=b"", tail=b"", extra=0, residue=0):
        self.rows = list(rows)
        R = self.R = len(self.rows)
        data = bytearray(lead)
        offsets = [len(data)]
        valid = []
        for r in self.rows:
            if r is None:
                valid.append(0)
            elif isinstance(r, tuple):
                valid.append(0)
                data += r[1]
            else:
                valid.append(1)
                data += r
            offsets.append(len(data))
        data += tail
        self.values = [r if isinstance(r, (bytes, bytearray)) else None for r in self.rows]
        for _ in range(extra):
            offsets.append(offsets[-1])
            valid.append(1)
        self.offsets = np.array(offsets, dtype=np.uint64)
        self.valid = np.array(valid, dtype=np.uint8)
        self.bytes_len = len(data)
        self.data = bytes(data)
        self.place(residue)

    def place(self, residue):
        """bytes at an address that is `residue` mod 16, at its exact size"""
        self._raw = np.zeros(self.bytes_len + 32, dtype=np.uint8)
        at = (residue - self._raw.ctypes.data) % 16
        self.bytes = self._raw[at:at + self.bytes_len]
        self.bytes[:] = np.frombuffer(self.data, dtype=np.uint8)
        assert self.bytes_len == 0 or self.bytes.ctypes.data % 16 == residue
        return self


def expected(col, specs, capacity=None, R=None):
    """(result fields, select fields, records) of the definition: records pre-filled, [p, k] written for k < R"""
    R = col.R if R is None else R
    capacity = col.R if capacity is None else capacity
    rec = np.zeros((len(specs), capacity), dtype=FIELD)
    rec.view(np.uint8)[:] = 0xA5
    n_matched = 0
    for p, s in enumerate(specs):
        for k in range(R):
            v = col.values[k]
            at = None if v is None else py_match(v, s)
            if at is None:
                rec[p, k] = (0, 0xFFFFFFFF, 0, 0, NO_SUCH_FIELD)
            else:
                rec[p, k] = (at, 0xFFFFFFFF, ord("l"), 0, 0)
                n_matched += 1
    res = dict(code=0, flags=0, n_rows=R, n_values=sum(v is not None for v in col.values[:R]), n_matched=n_matched,
               max_pieces=max(len(norm(s)[0]) for s in specs))
    sel = dict(code=0, n_documents=R, n_paths=len(specs), n_found=n_matched, n_no_bits=0)
    return res, sel, rec


def res_fields(r):
    return dict(code=r.code, flags=r.flags, n_rows=r.n_rows, n_values=r.n_values, n_matched=r.n_matched, max_pieces=r.max_pieces)


def sel_fields(s):
    return dict(code=s.code, n_documents=s.n_documents, n_paths=s.n_paths, n_found=s.n_found, n_no_bits=s.n_no_bits)


def run_twin(tw, col, specs, capacity=None, rows=None, n_rows=None, blocks=0, stage=0, bytes_len=None):
    """-> (rc, MatchResult, SelectResult, records[n_patterns, capacity]) of the twin; the outputs pre-filled"""
    capacity = col.R if capacity is None else capacity
    rows = col.R if rows is None else rows
    desc, data = flat(specs)
    rec = np.zeros((len(specs), max(capacity, 1)), dtype=FIELD)
    rec.view(np.uint8)[:] = 0xA5
    res, sel = MatchResult(), SelectResult()
    ctypes.memset(ctypes.byref(res), 0xA5, 48), ctypes.memset(ctypes.byref(sel), 0xA5, 48)
    d_n = None if n_rows is None else np.array([n_rows], dtype=np.uint64)
    blen = col.bytes_len if bytes_len is None else bytes_len
    rc = tw.msm_match_strings(1, desc.ctypes.data, data.ctypes.data, len(specs), col.offsets.ctypes.data,
                              col.valid.ctypes.data if col.valid.size else None, rows, ptr(d_n), col.bytes.ctypes.data if blen else None, blen,
                              rec.ctypes.data if capacity else None, capacity, ctypes.addressof(res), ctypes.addressof(sel), blocks, stage)
    return rc, res, sel, rec[:, :capacity]


def check_twin(tw, col, specs, brute=False, **kw):
    """The twin against the definition(s), over the whole outputs"""
    rc, res, sel, rec = run_twin(tw, col, specs, **kw)
    assert rc == 0
    want_res, want_sel, want_rec = expected(col, specs, capacity=kw.get("capacity"))
    assert res_fields(res) == want_res
    assert sel_fields(sel) == want_sel
    assert rec.tobytes() == want_rec.tobytes(), np.argwhere(rec != want_rec)[:8]
    if brute:
        for s in specs:
            for v in col.values:
                if v is not None:
                    assert brute_match(v, s) == py_match(v, s), (v, s)
    return res, sel, rec


def word(rng, n, alphabet=ALPHABET):
    return bytes(rng.choice(alphabet) for _ in range(n))


# ---- the pieces ---------------------------------------------------------------------------------------------------------------

def test_fold(tw):
    for c in range(256):
        assert tw.msm_fold1(c) == (c + 32 if 65 <= c <= 90 else c)
    rng = random.Random(1)
    edge = (0x40, 0x41, 0x5A, 0x5B, 0x60, 0x61, 0x7A, 0x7B, 0xC0, 0xC1, 0xDA, 0xDB, 0x00, 0xFF, 0x7F, 0x80)
    for _ in range(20000):
        b = [rng.choice(edge) if rng.random() < 0.7 else rng.randrange(256) for _ in range(4)]
        w = int.from_bytes(bytes(b), "little")
        assert tw.msm_fold4(w) == int.from_bytes(lower(bytes(b)), "little"), b


def test_fetch4(tw):
    lo, hi = 0x44332211, 0x88776655
    eight = (hi << 32 | lo).to_bytes(8, "little")
    for s in range(4):
        assert tw.msm_fetch4(lo, hi, s) == int.from_bytes(eight[s:s + 4], "little")


def test_word_at_every_residue_and_end(tw):
    for residue in range(16):
        for n in list(range(0, 36)) + [47, 48, 49]:
            col = Column([bytes(1 + (i % 250) for i in range(n))], residue=residue)
            if n:
                assert tw.msm_phase(col.bytes.ctypes.data) == residue
            for a in range(0, 96, 16):
                out = np.zeros(4, dtype=np.uint32)
                tw.msm_load_word16(col.bytes.ctypes.data, n, a, out.ctypes.data)
                want = bytes(col.data[c - residue] if 0 <= c - residue < n else 0 for c in range(a, a + 16))
                assert out.tobytes() == want, (residue, n, a)


def test_upper_bound(tw):
    off = np.array([0, 0, 0, 3, 3, 7, 7, 7, 9], dtype=np.uint64)
    for b in range(11):
        want = sum(1 for x in off if x <= b)
        assert tw.msm_upper_bound(off.ctypes.data, 0, len(off), b) == want


def test_compile_refuses(tw):
    def rc(specs, flags=0, n=None):
        desc, data = flat(specs)
        return tw.msm_compile(desc.ctypes.data, data.ctypes.data, len(specs) if n is None else n, flags, None)

    assert rc([b"a"]) == 0
    assert rc([b"a"] * 16) == 0
    assert rc([b"a"] * 17) == -1
    assert rc([], n=0) == -1
    assert rc([b"a"], flags=1) == -1
    assert rc([([b"a"], 8)]) == -1
    assert rc([([b"a", b""], 0)]) == -1
    assert rc([([b"a" * 256], 0)]) == -1
    assert rc([([b"a" * 255] * 4, 7)]) == 0
    assert rc([([b"a"] * 5, 0)]) == -1
    desc, data = flat([b"ab"])
    desc[0, 3] = 1  # a length behind n_pieces
    assert tw.msm_compile(desc.ctypes.data, data.ctypes.data, 1, 0, None) == -1
    desc[0, 3], desc[0, 0] = 0, 0
    assert tw.msm_compile(desc.ctypes.data, data.ctypes.data, 1, 0, None) == -1


# ---- named cases --------------------------------------------------------------------------------------------------------------

def test_named_cases(tw):
    L = lambda *pieces, f=0: (list(pieces), f)
    # a match that would span two rows is none
    _, _, rec = check_twin(tw, Column([b"xxab", b"cxx"]), [b"abc", b"ab", b"c"], brute=True)
    assert rec["code"][0].tolist() == [20, 20] and rec["bits"][1].tolist() == [2, 0] and rec["bits"][2].tolist() == [0, 0]
    # pieces do not overlap
    _, _, rec = check_twin(tw, Column([b"aaa", b"aaaa"]), [L(b"aa", b"aa")], brute=True)
    assert rec["code"][0].tolist() == [20, 0]
    _, _, rec = check_twin(tw, Column([b"ab", b"abb"]), [L(b"ab", b"b", f=AT_END)], brute=True)
    assert rec["code"][0].tolist() == [20, 0]
    _, _, rec = check_twin(tw, Column([b"a", b"aa", b"aba"]), [L(b"a", b"a")], brute=True)
    assert rec["code"][0].tolist() == [20, 0, 0]
    # both anchors: equality
    _, _, rec = check_twin(tw, Column([b"abc", b"abcd", b"xabc", b"ab", b""]), [L(b"abc", f=AT_START | AT_END)], brute=True)
    assert rec["code"][0].tolist() == [0, 20, 20, 20, 20]
    # the anchors alone, and the place that is reported
    _, _, rec = check_twin(tw, Column([b"abcabc", b"bcab", b"cab"]), [L(b"ab", f=AT_START), L(b"ab", f=AT_END), b"ab"], brute=True)
    assert rec["code"].tolist() == [[0, 20, 20], [20, 0, 0], [0, 0, 0]] and rec["bits"][1].tolist() == [0, 2, 1]
    # a piece longer than the row
    check_twin(tw, Column([b"ab", b"", b"abc"]), [b"abc", b"abcd", b"a" * 255], brute=True)
    # NOCASE: A-Z only
    rows = [b"AZ", b"az", b"@[", b"`{", b"\xc0\xe0", b"\xe0\xc0", b"aZ@"]
    _, _, rec = check_twin(tw, Column(rows), [L(b"az", f=NOCASE), L(b"AZ", f=NOCASE), L(b"@[", f=NOCASE), L(b"`{", f=NOCASE), L(b"\xe0", f=NOCASE),
                                               L(b"Az@", f=NOCASE | AT_START | AT_END)], brute=True)
    assert rec["code"][0].tolist() == [0, 0, 20, 20, 20, 20, 0] and rec["code"][2].tolist() == [20, 20, 0, 20, 20, 20, 20]
    assert rec["bits"][4].tolist() == [0, 0, 0, 0, 1, 0, 0] and rec["code"][5].tolist() == [20] * 6 + [0]
    # runs of empty and of null rows in front of a row whose first byte starts a match
    _, _, rec = check_twin(tw, Column([b"", b"", None, None, b"", b"abc", b"", None]), [b"abc", L(b"a", f=AT_START)], brute=True)
    assert rec["code"][0].tolist() == [20] * 5 + [0, 20, 20]
    # a null row with a non-zero length whose bytes hold the pattern
    _, _, rec = check_twin(tw, Column([b"x", ("null", b"abc"), b"y", ("null", b"ab"), b"c"], lead=b"abc", tail=b"abc"), [b"abc", b"b"])
    assert (rec["code"] == 20).all()


def test_bad_offsets_and_capacity(tw):
    col = Column([b"ab", b"cd", b"ef"])
    for k, v in ((1, 5), (2, 1), (3, 7)):  # descends once; an end past bytes_len
        bad = Column([b"ab", b"cd", b"ef"])
        bad.offsets[k] = v
        rc, res, sel, rec = run_twin(tw, bad, [b"a"])
        assert rc == 0 and res.code == BAD_ARGUMENT and sel.code == BAD_ARGUMENT
        assert (res.n_rows, res.n_values, res.n_matched, res.max_pieces) == (0, 0, 0, 0) and sel.n_documents == 0
        assert (rec.view(np.uint8) == 0xA5).all()
    # a violation at or past R is not looked at
    bad = Column([b"ab", b"cd", b"ef"], extra=2)
    bad.offsets[5] = 0
    rc, res, _, _ = run_twin(tw, bad, [b"a"], rows=5, n_rows=3, capacity=5)
    assert rc == 0 and res.code == 0 and res.n_rows == 3
    for kw in (dict(n_rows=4), dict(capacity=2), dict(n_rows=2**31, rows=3)):
        rc, res, sel, rec = run_twin(tw, col, [b"a"], **kw)
        assert rc == 0 and res.code == MSJ_CAPACITY and sel.code == MSJ_CAPACITY and res.n_rows == kw.get("n_rows", 3)
        assert (rec.view(np.uint8) == 0xA5).all()
    rc, res, sel, rec = run_twin(tw, col, [b"a", ([b"a", b"b"], 0)], n_rows=0)
    assert rc == 0 and res_fields(res) == dict(code=0, flags=0, n_rows=0, n_values=0, n_matched=0, max_pieces=2)
    assert sel_fields(sel) == dict(code=0, n_documents=0, n_paths=2, n_found=0, n_no_bits=0) and (rec.view(np.uint8) == 0xA5).all()


# ---- sweeps -------------------------------------------------------------------------------------------------------------------

def some_patterns(rng, text, n):
    """n patterns of 1 to 4 pieces, most cut from `text` so that they match somewhere"""
    out = []
    for _ in range(n):
        pieces = []
        for _ in range(rng.choice((1, 1, 2, 3, 4))):
            ln = rng.choice(PIECE_LENGTHS[:9])
            if text and rng.random() < 0.8:
                at = rng.randrange(len(text))
                x = text[at:at + ln]
            else:
                x = word(rng, ln)
            pieces.append(x or b"a")
        out.append((pieces, rng.choice((0, 0, AT_START, AT_END, NOCASE, AT_START | AT_END, NOCASE | AT_END, 7))))
    return out


def test_row_lengths_against_both_definitions(tw):
    rng = random.Random(7)
    c = constants(tw)
    lengths = list(range(19)) + list(range(62, 67))
    for trial in range(12):
        rows = []
        for ln in rng.sample(lengths, len(lengths)):
            r = rng.random()
            rows.append(None if r < 0.08 else ("null", word(rng, ln)) if r < 0.16 else word(rng, ln, ALPHABET[1:4] if trial % 2 else ALPHABET))
        col = Column(rows, lead=word(rng, trial % 3), tail=word(rng, trial % 5), residue=trial + 3)
        specs = some_patterns(rng, col.data, 16)
        check_twin(tw, col, specs, brute=True)
        check_twin(tw, col, specs[:3], blocks=1, stage=c["chunk"])
    for ln in (c["tile"] - 1, c["tile"], c["tile"] + 1):
        row = word(rng, ln, ALPHABET[1:4])
        col = Column([b"ab", row, b"", row[:40]], residue=5)
        specs = some_patterns(rng, row[-300:], 8) + [row[-255:], ([row[:255], row[-255:]], AT_START | AT_END)]
        check_twin(tw, col, specs)


def test_pieces_at_tile_borders(tw):
    """a piece of each length starting len - 1 .. 0 bytes in front of a tile border and ending 0 .. 1 bytes behind it, the
    border a row border too"""
    c = constants(tw)
    tile = c["tile"]
    rng = random.Random(3)
    for residue in (0, 1, 15):
        for ln in PIECE_LENGTHS:
            piece = bytes([0x62]) + word(rng, ln - 1, (0x61, 0x00, 0xFF))
            # byte b stands at coordinate b + residue: the border is byte tile - residue
            border = tile - residue
            starts = sorted({border - ln - 1, border - ln, border - ln + 1, border - ln + ln // 2, border - 1, border})
            data = bytearray(b"\x61" * (2 * tile))
            for which, s in enumerate(starts):
                d = bytearray(data)
                d[s:s + ln] = piece
                cuts = [0, border, len(d)] if which % 2 else [0, s, s + ln, len(d)]
                rows = [bytes(d[a:b]) for a, b in zip(cuts, cuts[1:])]
                col = Column(rows, residue=residue)
                specs = [piece, ([piece], AT_END), ([piece[:1], piece[-1:]], 0)]
                check_twin(tw, col, specs, blocks=1 + which % 3)


def test_more_rows_than_a_tile_stages(tw):
    c = constants(tw)
    rows = [b""] * (c["chunk"] + 3) + [b"abc"] + [None] * (c["stage"] + 5) + [b"xabc"] + [b"a", b"", b"bc"] * 100
    col = Column(rows, residue=9)
    specs = [b"abc", ([b"a", b"c"], 0), ([b"bc"], AT_END)]
    a = check_twin(tw, col, specs)
    b = check_twin(tw, col, specs, stage=c["chunk"])
    assert a[2].tobytes() == b[2].tobytes()


def test_every_position_a_hit(tw):
    c = constants(tw)
    col = Column([b"e" * 100, b"", b"e" * (c["tile"] + 17), None, b"e"], residue=2)
    _, _, rec = check_twin(tw, col, [b"e", ([b"e"], AT_END), ([b"e", b"e", b"e", b"e"], 0)])
    assert rec["bits"][0].tolist() == [0, 0, 0, 0, 0] and rec["bits"][1].tolist() == [99, 0, c["tile"] + 16, 0, 0]
