"""Substring patterns over a byte column on the device (msj_patterns_create and msj_match_strings_device,
csrc/match_strings_kernel.hip), through the C ABI.

Expected values come from the host twin of the same arithmetic (tests/match_strings_math_host.cpp), which
tests/test_match_strings_math.py holds against the definition written in Python, and from that definition itself
(``py_match``: ``re``; it shares nothing with the kernels).  Device output is compared with both over WHOLE tensors: the
records start from the fill 0xA5 with a canary behind the room, so a store at or past R shows; the two 48-byte results byte
for byte.

The kernel's constants as the shapes use them (``tmm.constants``): kTile = 8 192 start positions per tile, cut by address,
256 bytes of halo behind it, 32 positions per lane, 16-byte words.
"""
import ctypes
import random

import numpy as np
import pytest

from tests import test_match_strings_math as tmm

pytestmark = pytest.mark.gpu

CANARY = 16
MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
AT_START, AT_END, NOCASE = tmm.AT_START, tmm.AT_END, tmm.NOCASE
FLAG_NAMES = ((AT_START, "at_start"), (AT_END, "at_end"), (NOCASE, "nocase"))


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def tw():
    return tmm.load_twin()


def wrapper_specs(specs):
    """tmm's (pieces, flag bits) as ``compile_patterns`` takes them"""
    out = []
    for s in specs:
        pieces, flags = tmm.norm(s)
        out.append((pieces, {name for bit, name in FLAG_NAMES if flags & bit}))
    return out


class Held:
    """A column and a call's outputs on the device: the bytes at an address that is `residue` mod 16 with `junk` behind
    bytes_len, the records filled and with a canary behind the room"""

    def __init__(self, dev, col, n_patterns, capacity=None, residue=0, junk=b""):
        import torch

        self.dev, self.col, self.P = dev, col, n_patterns
        self.capacity = col.R if capacity is None else capacity
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev.device)
        self.d_offsets = up(col.offsets.view(np.int64))
        self.d_valid = up(col.valid if col.valid.size else np.zeros(1, dtype=np.uint8))
        image = np.frombuffer(b"\xEE" * residue + col.data + junk + b"\xEE" * 16, dtype=np.uint8).copy()
        self.raw = up(image)
        assert self.raw.data_ptr() % 16 == 0
        self.bytes_ptr = self.raw.data_ptr() + residue
        self.t_fields = torch.empty(((n_patterns * self.capacity + CANARY) * 2,), dtype=torch.int64, device=dev.device)
        self.t_res = torch.empty((48,), dtype=torch.uint8, device=dev.device)
        self.t_sel = torch.empty((48,), dtype=torch.uint8, device=dev.device)
        self.refill()

    def refill(self):
        self.t_fields.fill_(-0x5A5A5A5A5A5A5A5B), self.t_res.fill_(0xA5), self.t_sel.fill_(0xA5)

    def call(self, patterns, rows=None, d_n_rows=None, bytes_len=None, wait=True):
        import torch

        dev, col = self.dev, self.col
        blen = col.bytes_len if bytes_len is None else bytes_len
        rc = dev.lib.msj_match_strings_device(dev.ctx, patterns.handle, self.d_offsets.data_ptr(), self.d_valid.data_ptr(),
                                              col.R if rows is None else rows, None if d_n_rows is None else d_n_rows.data_ptr(),
                                              self.bytes_ptr if blen else None, blen, self.t_fields.data_ptr(), self.capacity,
                                              self.t_res.data_ptr(), self.t_sel.data_ptr(), dev._stream())
        if not wait or rc != 0:
            return rc
        torch.cuda.synchronize()
        return rc, self.out()

    def out(self):
        return self.t_fields.cpu().numpy().tobytes(), self.t_res.cpu().numpy().tobytes(), self.t_sel.cpu().numpy().tobytes()


def with_canary(rec, n_patterns, capacity):
    out = np.full((n_patterns * capacity + CANARY) * 16, 0xA5, dtype=np.uint8)
    out[:n_patterns * capacity * 16] = np.frombuffer(rec.tobytes(), dtype=np.uint8)
    return out.tobytes()


def run_match(dev, tw, col, specs, capacity=None, residue=0, junk=b"", definition=True, n_rows=None, rows=None):
    """One call on the device against the twin and the definition -> the twin's (result, select, records)"""
    import torch

    col.place(residue)
    capacity = col.R if capacity is None else capacity
    rc, want_res, want_sel, want_rec = tmm.run_twin(tw, col, specs, capacity=capacity, n_rows=n_rows, rows=rows)
    assert rc == 0
    if definition:
        d_res, d_sel, d_rec = tmm.expected(col, specs, capacity=capacity, R=n_rows)
        assert tmm.res_fields(want_res) == d_res and tmm.sel_fields(want_sel) == d_sel and want_rec.tobytes() == d_rec.tobytes()
    held = Held(dev, col, len(specs), capacity, residue, junk)
    patterns = dev.compile_patterns(wrapper_specs(specs))
    d_n = None if n_rows is None else torch.tensor([n_rows], dtype=torch.int64, device=dev.device)
    rc, (fields, res, sel) = held.call(patterns, rows=rows, d_n_rows=d_n)
    assert rc == 0
    assert tmm.res_fields(tmm.MatchResult.from_buffer_copy(res)) == tmm.res_fields(want_res)
    assert res == bytes(want_res) and sel == bytes(want_sel)
    got = np.frombuffer(fields, dtype=tmm.FIELD)
    want = np.frombuffer(with_canary(want_rec, len(specs), capacity), dtype=tmm.FIELD)
    assert fields == want.tobytes(), np.argwhere(got != want)[:8]
    return want_res, want_sel, want_rec


def piece_of(rng, ln):
    return b"b" + tmm.word(rng, ln - 1, (0x61, 0x00, 0xFF))


@pytest.mark.parametrize("ln", tmm.PIECE_LENGTHS)
def test_pieces_at_every_tile_border(dev, tw, ln):
    """a piece of `ln` bytes starting ln - 1 .. 0 bytes in front of a tile border and ending 0 .. 1 bytes in front of it: tile
    border j + 1 has the piece start x = j bytes in front of it, x = 0 .. ln + 1.  Three columns: one row; rows cut at the tile
    borders (a straddling piece is in no row); rows cut around every piece (the anchors hold)"""
    c = tmm.constants(tw)
    tile, residue = c["tile"], ln % 16
    rng = random.Random(ln)
    piece = piece_of(rng, ln)
    data = bytearray(b"a" * ((ln + 3) * tile))
    borders = [(j + 1) * tile - residue for j in range(ln + 2)]
    spans = []
    for x, border in enumerate(borders):
        data[border - x:border - x + ln] = piece
        spans.append((border - x, border - x + ln))
    specs = [piece, ([piece], AT_END), ([piece], AT_START | AT_END), ([piece[:1], piece[-1:]], 0)]
    cut = lambda at: [bytes(data[a:b]) for a, b in zip([0] + at, at + [len(data)])]
    for at in ([], borders, sorted({p for s in spans for p in s})):
        run_match(dev, tw, tmm.Column(cut(at)), specs, residue=residue)


@pytest.mark.parametrize("residue", range(16))
def test_pieces_at_word_borders_at_every_residue(dev, tw, residue):
    """the bytes' address is `residue` mod 16.  A piece of every length starting x bytes in front of a 16-byte word border, x =
    0 .. 17 and len - 1, len, len + 1: it starts at the border, straddles it by every split up to a word and a byte, ends at
    it, ends one byte in front of it.  Every placement has a border of its own.  Three columns: one row; rows cut at those
    word borders (a straddling piece is in no row, one that ends there holds AT_END, one that starts there AT_START); rows
    cut around every piece (both anchors hold)"""
    rng = random.Random(500 + residue)
    for ln in tmm.PIECE_LENGTHS:
        piece = piece_of(rng, ln)
        xs = sorted(set(range(18)) | {ln - 1, ln, ln + 1})
        stride = (2 * ln + 64) // 16 * 16
        data = bytearray(b"a" * (stride * (len(xs) + 1)))
        borders, spans = [], []
        for j, x in enumerate(xs):
            border = (j + 1) * stride - residue   # byte b stands at the address residue + b: a multiple of 16
            assert (border + residue) % 16 == 0 and border - x >= (borders[-1] if borders else 0)
            data[border - x:border - x + ln] = piece
            borders.append(border), spans.append((border - x, border - x + ln))
        specs = [piece, ([piece], AT_END), ([piece], AT_START), ([piece], AT_START | AT_END), ([piece[:1], piece[-1:]], AT_END)]
        cut = lambda at: [bytes(data[a:b]) for a, b in zip([0] + at, at + [len(data)])]
        for at in ([], borders, sorted({p for s in spans for p in s})):
            _, _, rec = run_match(dev, tw, tmm.Column(cut(at)), specs, residue=residue)
        assert int((rec["code"][3] == 0).sum()) == len(xs)   # (the last column: every piece is a row of its own)


@pytest.mark.parametrize("residue", range(16))
def test_word_borders_at_every_residue(dev, tw, residue):
    """short rows over the whole alphabet with bytes_len mod 16 = residue .. and pieces of every length cut from them"""
    rng = random.Random(100 + residue)
    rows = [None if rng.random() < 0.1 else tmm.word(rng, rng.choice((0, 1, 3, 15, 16, 17, 31, 33, 64))) for _ in range(40)]
    col = tmm.Column(rows, lead=tmm.word(rng, residue % 3), tail=tmm.word(rng, (5 * residue) % 16))
    specs = tmm.some_patterns(rng, col.data, 16)
    run_match(dev, tw, col, specs, residue=residue)


@pytest.mark.parametrize("mod", range(16))
def test_pattern_bytes_behind_bytes_len(dev, tw, mod):
    """bytes_len mod 16 = mod; the last row ends with the piece's first bytes and the piece goes on BEHIND bytes_len"""
    rng = random.Random(mod)
    for ln in (2, 5, 17, 255):
        piece = piece_of(rng, ln)
        keep = ln // 2
        body = b"a" * (64 + (mod - keep) % 16)
        col = tmm.Column([b"xyz", body + piece[:keep]])
        col.place(0)
        assert col.bytes_len % 16 == (3 + mod) % 16
        _, _, rec = run_match(dev, tw, col, [piece, ([piece[:keep]], AT_END)], junk=piece[keep:] + piece, residue=(3 * mod) % 16)
        assert rec["code"][0].tolist() == [20, 20] and rec["code"][1].tolist() == [20, 0]


def test_only_match_in_the_last_tile(dev, tw):
    c = tmm.constants(tw)
    row = bytearray(b"a" * (3 * c["tile"] + 1))
    row[-3:] = b"abX"
    _, _, rec = run_match(dev, tw, tmm.Column([b"ab", bytes(row), b""]), [b"bX", ([b"a", b"bX"], AT_END), ([b"X"], AT_START)], residue=7)
    assert rec["bits"][0].tolist() == [0, 3 * c["tile"] - 1, 0] and rec["code"][2].tolist() == [20, 20, 20]


def test_sixteen_patterns_and_one_per_call(dev, tw):
    rng = random.Random(16)
    text = b"".join(tmm.word(rng, 60, tmm.ALPHABET[1:4]) for _ in range(50))
    rows = [text[i:i + rng.randrange(0, 200)] for i in range(0, len(text) - 200, 37)]
    col = tmm.Column(rows)
    specs = tmm.some_patterns(rng, text, 16)
    for n in (1, 2, 3, 4):  # of 1 to 4 pieces each, in the text's order
        specs[n - 1] = ([text[a:a + 2] for a in sorted(rng.sample(range(0, 150), n))], 0)
    _, _, rec = run_match(dev, tw, col, specs, residue=3)
    for p, s in enumerate(specs):
        _, _, one = run_match(dev, tw, col, [s], residue=3)
        assert one[0].tobytes() == rec[p].tobytes()


def test_every_position_a_hit(dev, tw):
    c = tmm.constants(tw)
    col = tmm.Column([b"e" * 100, b"", b"e" * (2 * c["tile"] + 17), None, b"e"] + [b"ee"] * 300)
    _, _, rec = run_match(dev, tw, col, [b"e", ([b"e"], AT_END), ([b"e", b"e", b"e", b"e"], 0)], residue=11)
    assert (rec["bits"][0] == 0).all() and rec["bits"][1][2] == 2 * c["tile"] + 16


def test_rows_on_the_device_and_capacity(dev, tw):
    import torch

    col = tmm.Column([b"ab", b"cab", b"", None, b"abab"], extra=3)
    specs = [b"ab", ([b"a", b"b"], AT_END)]
    for R in (0, 1, 4, 5):
        run_match(dev, tw, col, specs, capacity=8, rows=8, n_rows=R)
    patterns = dev.compile_patterns(wrapper_specs(specs))
    for rows, capacity, R in ((8, 8, 9), (8, 4, 5), (4, 8, 5), (8, 8, 2**31)):
        held = Held(dev, col, 2, capacity)
        rc, (fields, res, sel) = held.call(patterns, rows=rows, d_n_rows=torch.tensor([R], dtype=torch.int64, device=dev.device))
        assert rc == 0
        r, s = tmm.MatchResult.from_buffer_copy(res), tmm.SelectResult.from_buffer_copy(sel)
        assert tmm.res_fields(r) == dict(code=MSJ_CAPACITY, flags=0, n_rows=R, n_values=0, n_matched=0, max_pieces=0) and r.reserved == 0
        assert tmm.sel_fields(s) == dict(code=MSJ_CAPACITY, n_documents=0, n_paths=0, n_found=0, n_no_bits=0)
        assert fields == b"\xA5" * len(fields)


def test_hostile_offsets(dev, tw):
    specs = [b"a", ([b"a", b"b"], 0)]
    patterns = dev.compile_patterns(wrapper_specs(specs))
    for k, v in ((1, 5), (2, 1), (3, 7), (0, 2**63)):
        col = tmm.Column([b"ab", b"cd", b"ef"])
        col.offsets[k] = v
        rc, want_res, want_sel, _ = tmm.run_twin(tw, col, specs)
        assert rc == 0 and want_res.code == BAD_ARGUMENT
        rc, (fields, res, sel) = Held(dev, col, 2).call(patterns)
        assert rc == 0 and res == bytes(want_res) and sel == bytes(want_sel)
        assert fields == b"\xA5" * len(fields)


def test_bad_arguments_in_their_order(dev):
    import torch

    lib, ctx = dev.lib, dev.ctx
    col = tmm.Column([b"ab", b"c"])
    held = Held(dev, col, 1)
    pats = dev.compile_patterns([b"a"])
    off, val, byt, fld, res, sel = (held.d_offsets.data_ptr(), held.d_valid.data_ptr(), held.bytes_ptr, held.t_fields.data_ptr(),
                                    held.t_res.data_ptr(), held.t_sel.data_ptr())
    st = dev._stream()

    def call(**kw):
        a = dict(ctx=ctx, patterns=pats.handle, off=off, val=val, rows=2, n=None, byt=byt, blen=3, fld=fld, cap=2, res=res, sel=sel)
        a.update(kw)
        return lib.msj_match_strings_device(a["ctx"], a["patterns"], a["off"], a["val"], a["rows"], a["n"], a["byt"], a["blen"], a["fld"],
                                            a["cap"], a["res"], a["sel"], st)

    assert call() == 0
    for kw in (dict(ctx=None), dict(patterns=None), dict(res=None), dict(sel=None), dict(off=None), dict(val=None), dict(fld=None),
               dict(byt=None), dict(sel=res), dict(fld=fld + 8), dict(off=off + 4), dict(n=off + 4), dict(res=res + 4), dict(sel=sel + 4)):
        assert call(**kw) == BAD_ARGUMENT, kw
    for kw in (dict(rows=1 << 40), dict(cap=1 << 40), dict(blen=1 << 40)):
        assert call(**kw) == MSJ_CAPACITY, kw
    # which error wins: a NULL array over a size of 2^40, that over an alignment
    assert call(off=None, rows=1 << 40) == BAD_ARGUMENT
    assert call(rows=1 << 40, fld=fld + 8) == MSJ_CAPACITY
    # what is allowed: no rows and no bytes with NULL arrays, bytes and valid at any address
    assert call(off=None, val=None, rows=0, byt=None, blen=0, fld=None, cap=0) == 0
    assert call(byt=byt + 1, blen=2, val=val + 1, rows=1, cap=1) == 0
    torch.cuda.synchronize()
    # msj_patterns_create
    h = ctypes.c_void_p()
    from mojo_simdjson_amd import _lib

    buf = ctypes.create_string_buffer(b"abcd", 4)
    one = lambda n_pieces=1, flags=0, lens=(4, 0, 0, 0), ptr=ctypes.addressof(buf): _lib.MsjPattern(ptr, n_pieces, flags, (ctypes.c_uint32 * 4)(*lens))
    table = lambda *p: (_lib.MsjPattern * len(p))(*p)
    assert lib.msj_patterns_create(None, table(one()), 1, 0, ctypes.byref(h)) == BAD_ARGUMENT
    assert lib.msj_patterns_create(ctx, table(one()), 1, 0, None) == BAD_ARGUMENT
    for bad in (one(0), one(5), one(flags=8), one(lens=(0, 0, 0, 0)), one(lens=(256, 0, 0, 0)), one(lens=(4, 1, 0, 0)), one(2, lens=(2, 0, 0, 0)),
                one(ptr=None)):
        assert lib.msj_patterns_create(ctx, table(bad), 1, 0, ctypes.byref(h)) == BAD_ARGUMENT
    assert lib.msj_patterns_create(ctx, table(one()), 0, 0, ctypes.byref(h)) == BAD_ARGUMENT
    assert lib.msj_patterns_create(ctx, table(*[one()] * 17), 17, 0, ctypes.byref(h)) == BAD_ARGUMENT
    assert lib.msj_patterns_create(ctx, table(one()), 1, 1, ctypes.byref(h)) == BAD_ARGUMENT
    assert lib.msj_patterns_create(ctx, None, 1, 0, ctypes.byref(h)) == BAD_ARGUMENT
    assert lib.msj_patterns_create(ctx, table(one(4, 7, (1, 1, 1, 1))), 1, 0, ctypes.byref(h)) == 0
    lib.msj_patterns_destroy(h)
    lib.msj_patterns_destroy(None)
    for spec in ("", b"", ([], ()), ([b"a"] * 5, ()), ([b"a"], {"upper"}), ([b"a" * 256], ()), 7):
        with pytest.raises(ValueError):
            dev.compile_patterns([spec])
    with pytest.raises(ValueError):
        dev.compile_patterns([b"a"] * 17)


def test_wrapper_on_its_own_tensors(dev, tw):
    """``Stage1Device.match_strings`` with the caller's tensors and sync=False, R from a tensor"""
    import torch

    col = tmm.Column([b"GET /a.png", b"get /b.PNG", None, b"POST /a.png", b""], extra=2)
    specs = [b"png", ([b"GET ", b".png"], AT_START | AT_END | NOCASE)]
    want_res, want_sel, want_rec = tmm.expected(col, specs, capacity=7)
    up = lambda a: torch.from_numpy(np.array(a)).to(dev.device)
    d_fields = torch.full((2, 7, 2), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev.device)
    d_n = torch.tensor([5], dtype=torch.int64, device=dev.device)
    d_res, got_fields, d_sel = dev.match_strings(dev.compile_patterns(wrapper_specs(specs)), up(col.offsets.view(np.int64)), up(col.valid),
                                                 up(np.frombuffer(col.data, dtype=np.uint8)), d_n_rows=d_n, d_fields=d_fields, sync=False)
    assert got_fields is d_fields and d_res.dtype == torch.uint8
    assert tmm.res_fields(tmm.MatchResult.from_buffer_copy(d_res.cpu().numpy().tobytes())) == want_res
    assert tmm.sel_fields(tmm.SelectResult.from_buffer_copy(d_sel.cpu().numpy().tobytes())) == want_sel
    assert d_fields.cpu().numpy().tobytes() == want_rec.tobytes()
    res, fields, _ = dev.match_strings(dev.compile_patterns([b"png", "a.p"]), up(col.offsets.view(np.int64))[:6], up(col.valid),
                                       up(np.frombuffer(col.data, dtype=np.uint8)))
    assert (res.code, res.n_rows, res.n_values, res.n_matched, res.max_pieces) == (0, 5, 4, 4, 1) and tuple(fields.shape) == (2, 5, 2)
