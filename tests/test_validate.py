"""Stage 2's verdict on the device (msj_validate_device, csrc/validate_kernel.hip) through the C ABI.

Expected values come from the host twin of the same rule (tests/validate_math_host.cpp), which tests/test_validate_math.py
holds against a serial walker and against Python's json on this corpus.  Two ways in: the real chain on the device
(stage 1, stage2_prep with partners, number_values, validate), and -- for the corpus of several hundred thousand small
documents -- token arrays built on the host by the oracles, uploaded together and judged by one call per document with
nothing waited for in between.  DERIVED like the token arrays: the definition is include/msj_stage1.h's.
"""
import ctypes
import random

import numpy as np
import pytest

from tests import helpers
from tests import test_number_math as tnm
from tests import test_validate_math as tvm

pytestmark = pytest.mark.gpu

UINT64_MAX = tvm.UINT64_MAX
BLOCK = 1024  # tokens per workgroup of val_tokens (csrc/validate_kernel.hip: kBlock)


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
def twin():
    return tvm.load_twin()


@pytest.fixture(scope="module")
def nm():
    return tnm.load_twin()


def host_arrays(oracle, nm, data):
    """What stage 1 + msj_stage2_prep_device(match) + msj_number_values_device leave for `data`, from the oracles:
    (idx, type, depth, match, end, flags, numbers first_error), or the stage-1 code when that is not 0."""
    rc, n, idx = helpers.run_oracle(oracle.msj_oracle_stage1, data)
    if rc != 0:
        return rc
    idx = idx[:n].copy()
    typ, depth, _ = helpers.oracle_tokens(data, idx)
    match = helpers.oracle_match(typ)
    end, flags = helpers.oracle_token_spans(data, idx)
    return idx, typ, depth, match, end, flags, tvm.numbers_first_error(nm, data, idx, flags)


def twin_of(twin, data, arrays, max_depth=100, numbers=True):
    idx, typ, depth, match, end, flags, fe = arrays
    return tvm.twin_validate(twin, data, idx, typ, depth, match, end, flags, fe if numbers else None, max_depth)


def quad(r):
    return (r.code, r.error_token, r.error_offset, r.flags)


def device_document(dev, data, max_depth=100):
    """The real chain on the device."""
    import torch

    d_buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev.device)
    return dev.validate_document(d_buf, len(data), max_depth)


def check_document(dev, oracle, twin, nm, data, max_depth=100, where=None):
    """Chain on the device against the twin on the oracles' arrays; -> the device result (or stage 1's code)."""
    arrays = host_arrays(oracle, nm, data)
    got = device_document(dev, data, max_depth)
    if isinstance(arrays, int):
        assert got == arrays, (where, got, arrays)
        return got
    want = twin_of(twin, data, arrays, max_depth)
    assert not isinstance(got, int), (where, got)
    assert quad(got) == quad(want), (where, quad(got), quad(want), data[:120])
    assert got.n_escaped == want.n_escaped, where
    return got


def run_batch(dev, twin, items):
    """items: (data, host arrays, max_depth, numbers) per document.  All token arrays in one upload (every slice on the
    16-byte grid), one msj_validate_device per document on one stream with nothing waited for, the results read once;
    each equal to the twin's on the same arrays.  -> list of (code, token)."""
    import torch
    from mojo_simdjson_amd import _lib

    def up16(x):
        return (x + 15) & ~15

    tok_total = sum(up16(len(a[0])) for _, a, _, _ in items)
    byte_total = sum(len(d) for d, _, _, _ in items)
    h_buf = np.zeros(max(byte_total, 1), dtype=np.uint8)
    h_idx, h_match, h_end = (np.zeros(tok_total, dtype=np.uint32) for _ in range(3))
    h_depth = np.zeros(tok_total, dtype=np.int32)
    h_type, h_flags = (np.zeros(tok_total, dtype=np.uint8) for _ in range(2))
    h_num = np.zeros((len(items), 4), dtype=np.uint64)
    t = b = 0
    place = []
    for k, (data, (idx, typ, depth, match, end, flags, fe), _, _) in enumerate(items):
        n = len(idx)
        h_buf[b:b + len(data)] = np.frombuffer(data, dtype=np.uint8)
        h_idx[t:t + n], h_type[t:t + n], h_depth[t:t + n] = idx, typ, depth
        h_match[t:t + n], h_end[t:t + n], h_flags[t:t + n] = match, end, flags
        h_num[k] = (0, 0 if fe == UINT64_MAX else 1, fe, 0)
        place.append((b, t, n))
        b += len(data)
        t += up16(n)
    dv = dev.device
    d_buf, d_idx, d_type, d_depth, d_match, d_end, d_flags, d_num = (
        torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else (x.view(np.int64) if x.dtype == np.uint64 else x)).to(dv)
        for x in (h_buf, h_idx, h_type, h_depth, h_match, h_end, h_flags, h_num))
    d_res = torch.zeros((len(items), 32), dtype=torch.uint8, device=dv)
    stream = dev._stream()
    for k, ((data, _, max_depth, numbers), (b, t, n)) in enumerate(zip(items, place)):
        rc = dev.lib.msj_validate_device(dev.ctx, d_buf.data_ptr() + b, len(data), d_idx.data_ptr() + 4 * t, n, d_type.data_ptr() + t,
                                         d_depth.data_ptr() + 4 * t, d_match.data_ptr() + 4 * t, d_end.data_ptr() + 4 * t,
                                         d_flags.data_ptr() + t, (d_num.data_ptr() + 32 * k) if numbers else None, max_depth,
                                         d_res.data_ptr() + 32 * k, stream)
        assert rc == 0, rc
    raw = d_res.cpu().numpy().tobytes()
    out = []
    for k, (data, arrays, max_depth, numbers) in enumerate(items):
        got = _lib.MsjValidateResult.from_buffer_copy(raw[32 * k:32 * k + 32])
        want = twin_of(twin, data, arrays, max_depth, numbers)
        assert quad(got) == quad(want), (data[:120], max_depth, numbers, quad(got), quad(want))
        assert got.n_escaped == want.n_escaped
        out.append((got.code, got.error_token))
    return out


def batched(dev, oracle, twin, nm, docs, chunk=20000):
    """docs: iterable of (data, max_depth, numbers); documents whose stage 1 is not 0 are left out.  -> code histogram"""
    codes, items = {}, []

    def flush():
        for code, _ in run_batch(dev, twin, items):
            codes[code] = codes.get(code, 0) + 1
        items.clear()

    for data, max_depth, numbers in docs:
        arrays = host_arrays(oracle, nm, data)
        if isinstance(arrays, int):
            continue
        items.append((data, arrays, max_depth, numbers))
        if len(items) >= chunk:
            flush()
    if items:
        flush()
    return codes


def test_cpu_corpus_batched(dev, oracle, twin, nm):
    """The corpus of tests/test_validate_math.py: (code, error_token, error_offset, flags) equal to the twin's."""
    def docs():
        for s in tvm.small_strings():
            yield s, 3, True
        for doc, mut in tvm.seeded_documents(20260, 200000):
            yield mut, 100, True
            yield mut, 3, len(mut) % 2 == 0  # (about every other one with d_numbers == NULL)
        for body in tvm.escape_cases():
            yield tvm._string_doc(body), 100, True
    codes = batched(dev, oracle, twin, nm, docs())
    assert sum(codes.values()) > 400000, codes
    for c in (tvm.SUCCESS, tvm.TAPE, tvm.DEPTH, tvm.STRING, tvm.T_ATOM, tvm.F_ATOM, tvm.N_ATOM, tvm.NUMBER):
        assert codes.get(c, 0) > 0, codes


def _filler(tokens):
    """`tokens` tokens that leave an array expecting a value: '1,' pairs, an empty array in front for an odd count"""
    assert tokens >= 0 and tokens != 1
    if tokens % 2:
        return b"[]," + b"1," * ((tokens - 3) // 2)
    return b"1," * (tokens // 2)


# what is planted at token p (the filler in front makes it land there), and the max_depth it is judged with
PLANTS = [
    ("tape", lambda f: b"[" + f + b",1,1]", 100),                 # a comma where a value belongs
    ("depth", lambda f: b"[" + f + b"[1],1]", 2),                 # a non-empty array at walker depth 2
    ("string", lambda f: b"[" + f + b'"a\\qb",1]', 100),
    ("pair", lambda f: b"[" + f + b'"\\ud800x",1]', 100),
    ("t_atom", lambda f: b"[" + f + b"tru,1]", 100),
    ("f_atom", lambda f: b"[" + f + b"fals,1]", 100),
    ("n_atom", lambda f: b"[" + f + b"nul,1]", 100),
    ("number", lambda f: b"[" + f + b"01,1]", 100),
    # the partner on the far side of the border: ']' lands at p - 1 (filler two tokens shorter: its last ',' dropped)
    ("valid_after_partner", lambda f: b'{"a":[' + f[:-1] + b'],"b":2}', 100),
    ("no_comma_after_partner", lambda f: b'{"a":[' + f[:-1] + b'] "b":2}', 100),
    ("key_by_partner", lambda f: b'{"a":[' + f[:-1] + b'],"b" 2}', 100),
    ("no_key_by_partner", lambda f: b'[[' + f[:-1] + b'],"b":2]', 100),
    ("key_wanted_by_partner", lambda f: b'{"a":[' + f[:-1] + b"],2:3}", 100),
    ("wrong_closer", lambda f: b"[[" + f[:-1] + b"},1]", 100),
]


def test_block_and_halo_borders(dev, oracle, twin, nm):
    """An error of every kind planted at every token position of a window of two blocks + 8 tokens around a block border:
    the neighbours i-1 .. i-3 of the block's first tokens come from the halo, the partner from the far side."""
    want_code = {"tape": tvm.TAPE, "depth": tvm.DEPTH, "string": tvm.STRING, "pair": tvm.STRING, "t_atom": tvm.T_ATOM,
                 "f_atom": tvm.F_ATOM, "n_atom": tvm.N_ATOM, "number": tvm.NUMBER, "valid_after_partner": tvm.SUCCESS,
                 "no_comma_after_partner": tvm.TAPE, "key_by_partner": tvm.TAPE, "no_key_by_partner": tvm.TAPE,
                 "key_wanted_by_partner": tvm.TAPE, "wrong_closer": tvm.TAPE}
    # where the error sits relative to p (the token behind the far partner's closing bracket)
    shift = {"key_by_partner": 2, "no_key_by_partner": 2, "key_wanted_by_partner": 1, "wrong_closer": -1}
    window = range(BLOCK - 4, 3 * BLOCK + 4)
    for name, make, max_depth in PLANTS:
        head = make(b"1,")
        front = 4 if head.startswith(b'{"a":[') else (2 if head.startswith(b"[[") else 1)  # tokens in front of the filler
        items = []
        for p in window:
            data = make(_filler(p - front))
            items.append((data, host_arrays(oracle, nm, data), max_depth, True))
        out = run_batch(dev, twin, items)
        for (code, token), p in zip(out, window):
            assert code == want_code[name], (name, p, code, token)
            assert token == (p + shift.get(name, 0) if code else UINT64_MAX), (name, p, token)


@pytest.mark.parametrize("workload", ["minified", "utf8", "pretty4"])
def test_workloads_1mib(dev, oracle, twin, nm, workload):
    """Valid as generated; then one seeded single-byte edit at each of 1 000 places: equal to the twin."""
    from mojo_simdjson_amd import synth

    u = synth.workload(workload, 1 << 20).tobytes()
    res = check_document(dev, oracle, twin, nm, u, where=workload)
    assert quad(res) == (0, UINT64_MAX, UINT64_MAX, 0)
    assert res.n_escaped > 100
    rng = random.Random(workload)
    codes = {}
    for k in range(1000):
        b = bytearray(u)
        b[rng.randrange(len(b))] = rng.choice(tvm.EDIT_ALPHABET)
        got = check_document(dev, oracle, twin, nm, bytes(b), where=(workload, k))
        c = got if isinstance(got, int) else got.code
        codes[c] = codes.get(c, 0) + 1
    assert len(codes) >= 3, codes


def test_minified_1gib(dev, oracle):
    """1 GiB as ONE document ([unit,unit,...,last] of a 64 MiB unit and a small last element): 0 with flags == 0 (the root
    is wide enough for the count pass to run); then single bytes changed near the start, in the middle and in the last 100 bytes: the planted token and
    code, found by the call alone; two plants at once report the earlier."""
    import torch

    from mojo_simdjson_amd import synth

    u = synth.workload("minified", 64 << 20)
    ub = u.tobytes()
    rc, n_unit, uidx = helpers.run_oracle(oracle.msj_oracle_stage1, ub)
    assert rc == 0
    uidx = uidx[:n_unit]
    utyp = u[uidx]
    reps = 16
    d_unit = torch.from_numpy(u).to(dev.device)
    sep = torch.tensor([ord(",")], dtype=torch.uint8, device=dev.device)
    parts = [torch.tensor([ord("[")], dtype=torch.uint8, device=dev.device)]
    for r in range(reps):
        parts += [d_unit, sep] if r + 1 < reps else [d_unit]
    tail = b',{"end":true,"s":"a\\nb"}]'  # the last 100 bytes of a unit are padding: the document's own last element is edited
    parts.append(torch.from_numpy(np.frombuffer(tail, dtype=np.uint8).copy()).to(dev.device))
    d_buf = torch.cat(parts)
    length = d_buf.numel()
    assert length > (1 << 30) - (1 << 20)  # (a unit is a few bytes short of 64 MiB)
    tail_off, tail_tok = 1 + reps * len(ub) + reps - 1, 1 + reps * n_unit + reps - 1  # the ',' in front of the last element
    n = tail_tok + 11
    assert length == tail_off + len(tail) and len(tail) < 100
    res = dev.validate_document(d_buf, length)
    assert quad(res) == (0, UINT64_MAX, UINT64_MAX, 0), quad(res)

    def where(rep, local_token):
        """(byte offset, token index) in the big document of token `local_token` of unit `rep`"""
        return 1 + rep * (len(ub) + 1) + int(uidx[local_token]), 1 + rep * (n_unit + 1) + local_token

    colons = np.nonzero(utyp == ord(":"))[0]
    trues = np.array([t for t in np.nonzero(utyp == ord("t"))[0][:5000] if ub[uidx[t]:uidx[t] + 4] == b"true"])
    # a "\n" escape (an odd run of backslashes in front of the n) and the string token it sits in
    esc = []
    pos = ub.find(b"\\n")
    while pos >= 0 and len(esc) < 3:
        if ub[pos - 1] != 0x5C:
            tok = int(np.searchsorted(uidx, pos, side="right")) - 1
            if utyp[tok] == ord('"'):
                esc.append((pos, tok))
        pos = ub.find(b"\\n", pos + 2)
    assert colons.size and trues.size and esc

    plants = []  # (offset of the changed byte, new byte, token, code, offset of the token)
    for rep, pick in ((0, 0), (reps // 2, len(colons) // 2)):
        off, tok = where(rep, int(colons[pick]))
        plants.append((off, ord(","), tok, tvm.TAPE, off))
        off, tok = where(rep, int(trues[min(pick, trues.size - 1)]))
        plants.append((off + 3, ord("x"), tok, tvm.T_ATOM, off))
        epos, etok = esc[0]
        off, tok = where(rep, etok)
        plants.append((off + (epos - int(uidx[etok])) + 1, ord("q"), tok, tvm.STRING, off))
    # the last 100 bytes: , { "end" : true , "s" : "a\nb" } ] are tokens tail_tok .. tail_tok + 10
    assert tail[8:12] == b"true" and tail[19:21] == b"\\n" and tail[7:8] == b":"
    plants.append((tail_off + 20, ord("q"), tail_tok + 8, tvm.STRING, tail_off + 17))
    plants.append((tail_off + 11, ord("x"), tail_tok + 4, tvm.T_ATOM, tail_off + 8))
    plants.append((tail_off + 7, ord(","), tail_tok + 3, tvm.TAPE, tail_off + 7))
    for off, byte, tok, code, tok_off in plants:
        old = int(d_buf[off])
        d_buf[off] = byte
        res = dev.validate_document(d_buf, length)
        d_buf[off] = old
        assert quad(res) == (code, tok, tok_off, 0), (off, quad(res), tok, code)
        assert res.error_token < n
    # two at once: the earlier wins, whatever its kind
    (o1, b1, t1, c1, _), (o2, b2, t2, c2, _) = plants[1], plants[-1]
    old1, old2 = int(d_buf[o1]), int(d_buf[o2])
    d_buf[o1], d_buf[o2] = b1, b2
    res = dev.validate_document(d_buf, length)
    assert (res.code, res.error_token) == (c1, t1)
    d_buf[o1] = old1
    (o3, b3, t3, c3, _) = plants[3]
    old3 = int(d_buf[o3])
    d_buf[o3] = b3
    res = dev.validate_document(d_buf, length)
    assert (res.code, res.error_token) == (c3, t3)
    d_buf[o3], d_buf[o2] = old3, old2
    assert quad(dev.validate_document(d_buf, length)) == (0, UINT64_MAX, UINT64_MAX, 0)


def test_element_count(dev, oracle, twin, nm):
    """0xFFFFFF elements pass, 0x1000000 are MSJ_CAPACITY at the closing bracket; more than 64 candidates: clipped."""
    exact = b"[" + b"1," * (0xFFFFFF - 1) + b"1]"
    over = b"[" + b"1," * 0xFFFFFF + b"1]"
    n_over = 2 * 0x1000000 + 1
    r = check_document(dev, oracle, twin, nm, exact, where="exact")
    assert quad(r) == (0, UINT64_MAX, UINT64_MAX, 0)
    r = check_document(dev, oracle, twin, nm, over, where="over")
    assert quad(r) == (tvm.CAPACITY, n_over - 1, len(over) - 1, 0)
    doc = b'{"a":' + over + b"}"
    r = check_document(dev, oracle, twin, nm, doc, where="object")
    assert quad(r) == (tvm.CAPACITY, 3 + n_over - 1, 5 + len(over) - 1, 0)
    doc = b"[" * 10 + over + b"]" * 10
    r = check_document(dev, oracle, twin, nm, doc, where="nested")
    assert quad(r) == (tvm.CAPACITY, 10 + n_over - 1, 10 + len(over) - 1, 0)
    doc = b"[" * 70 + over + b"]" * 70  # 71 candidates
    r = check_document(dev, oracle, twin, nm, doc, max_depth=100, where="clipped")
    assert quad(r) == (0, UINT64_MAX, UINT64_MAX, tvm.COUNTS_CLIPPED)


def _body(length, unit, bad_at):
    """An escaped body of exactly `length` bytes made of `unit` (starts with an escape) and 'x' padding; bad_at: None, or
    which escape ('first', 'middle', 'last') becomes \\q"""
    k = length // len(unit)
    units = [unit] * k
    if bad_at is not None:
        j = {"first": 0, "middle": k // 2, "last": k - 1}[bad_at]
        units[j] = b"\\q" + unit[2:]
    return b"".join(units) + b"x" * (length - k * len(unit))


@pytest.mark.parametrize("length", [1023, 1024, 1025, 1026, 4096, 4097, 70000, 1 << 20, (1 << 20) + 1, (1 << 20) + 4097, 3 << 20])
def test_long_escaped_bodies(dev, oracle, twin, nm, length):
    """Bodies walked by their lane (<= 1024 bytes), by a wave (<= 1 MiB) and by the grid, the bad escape first, last and
    in the middle.  The units repeat from the body's first byte, so the 5- and 7-byte ones reach every phase of the 64-byte
    steps, but a surrogate pair only ever starts at a multiple of 4 (12 j mod 64), and the damaged pairs sit at j = 0, k // 2
    and k - 1: three phases.  Every kind of escape at every phase, in front of the closing quote and around the 4 KiB piece
    borders of a body over 1 MiB is tests/test_escape_phases.py."""
    pair = b"\\ud83d\\ude00"
    for unit in (b"\\nab", b"\\\\\\tq", pair, b"\\u00e9z"):
        for bad_at in (None, "first", "middle", "last"):
            doc = b'{"k":["' + _body(length, unit, bad_at) + b'",tru]}'
            r = check_document(dev, oracle, twin, nm, doc, where=(length, unit, bad_at))
            assert (r.code, r.error_token) == ((tvm.T_ATOM, 6) if bad_at is None else (tvm.STRING, 4)), (length, unit, bad_at)
    k = length // 12
    for j in (0, k // 2, k - 1):  # one half of one pair damaged
        for half, repl in ((0, b"\\ue83d"), (6, b"\\ufe00"), (6, b"x\\de00"[:6])):
            body = bytearray(pair * k + b"y" * (length - 12 * k))
            body[12 * j + half:12 * j + half + 6] = repl
            doc = b'["' + bytes(body) + b'"]'
            r = check_document(dev, oracle, twin, nm, doc, where=(length, j, half))
            assert (r.code, r.error_token) == (tvm.STRING, 1)


@pytest.mark.parametrize("length", [1025, 70000, 1 << 20, 3 << 20])
def test_one_run_of_backslashes(dev, oracle, twin, nm, length):
    """Bodies that are a single run of 2k and 2k + 1 backslashes, valid and with one bad escape behind the run, by the wave
    and by the grid: the right verdict, in time linear in the body (the parity of a run is carried from step to step,
    not walked back to from every backslash)."""
    import time

    import torch

    t0 = time.perf_counter()
    for body, bad in tvm.backslash_run_bodies(length):
        doc = b'["' + body + b'",tru]'
        r = check_document(dev, oracle, twin, nm, doc, where=(length, body[-16:]))
        assert (r.code, r.error_token) == ((tvm.STRING, 1) if bad else (tvm.T_ATOM, 3)), (length, body[-16:], bad)
    torch.cuda.synchronize()
    # 12 documents of at most 3 MiB: milliseconds on the device, the rest is the host's oracles
    assert time.perf_counter() - t0 < 60


def test_numbers_given_or_null(dev, oracle, twin, nm):
    import torch

    data = b"[1,01]"
    arrays = host_arrays(oracle, nm, data)
    out = run_batch(dev, twin, [(data, arrays, 100, True), (data, arrays, 100, False)])
    assert out == [(tvm.NUMBER, 3), (0, UINT64_MAX)]
    # the device chain, by hand
    d_buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev.device)
    d_idx = torch.empty(len(data) + 7, dtype=torch.int32, device=dev.device)
    d_carry = dev.new_carry()
    dev.index(d_buf, d_idx, d_carry)
    n = int(dev.fetch(d_carry).count)
    d_type, d_depth, _, d_match, d_end, d_flags = dev.stage2_prep(d_buf, len(data), d_idx, n, match=True)
    r = dev.validate(d_buf, len(data), d_idx, n, d_type, d_depth, d_match, d_end, d_flags, None)
    assert quad(r) == (0, UINT64_MAX, UINT64_MAX, tvm.NUMBERS_UNCHECKED)
    _, d_num = dev.number_values(d_buf, len(data), d_idx, n, d_flags, sync=False)
    r = dev.validate(d_buf, len(data), d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_num)
    assert quad(r) == (tvm.NUMBER, 3, 3, 0)


def test_bad_arguments_launch_nothing(dev):
    import torch

    data = b"[1,2]"
    d_buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev.device)
    d_idx = torch.empty(16, dtype=torch.int32, device=dev.device)
    d_carry = dev.new_carry()
    dev.index(d_buf, d_idx, d_carry)
    n = int(dev.fetch(d_carry).count)
    d_type, d_depth, _, d_match, d_end, d_flags = dev.stage2_prep(d_buf, len(data), d_idx, n, match=True)
    d_res = torch.full((32,), 0xAB, dtype=torch.uint8, device=dev.device)
    tensors = {1: d_buf, 3: d_idx, 5: d_type, 6: d_depth, 7: d_match, 8: d_end, 9: d_flags, 12: d_res}  # by argument position
    good = [dev.ctx, None, len(data), None, n, None, None, None, None, None, None, 100, None, dev._stream()]
    for k, t in tensors.items():
        good[k] = ctypes.c_void_p(t.data_ptr())

    def call(change=None):
        a = list(good)
        for k, v in (change or {}).items():
            a[k] = v
        return dev.lib.msj_validate_device(*a)

    assert call({4: 0}) == -1 and call({11: 0}) == -1  # n == 0, max_depth == 0
    for k in (0, 1, 3, 5, 6, 7, 8, 9, 12):
        assert call({k: None}) == -1, k
    for k, off in ((3, 4), (6, 4), (7, 8), (8, 4), (5, 4), (9, 1), (12, 4)):  # off the 16-byte / 8-byte grid
        assert call({k: ctypes.c_void_p(tensors[k].data_ptr() + off)}) == -1, k
    assert call({10: ctypes.c_void_p(d_res.data_ptr() + 4)}) == -1
    assert call({2: 1 << 32}) == 1 and call({4: 1 << 31}) == 1  # MSJ_CAPACITY
    torch.cuda.synchronize()
    assert (d_res.cpu().numpy() == 0xAB).all()  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert d_res[:4].cpu().numpy().view(np.int32)[0] == 0


def test_chain_without_waiting(dev, oracle, twin, nm):
    """index -> stage2_prep(match) -> number_values -> validate, every result left on the device, read once at the end."""
    import torch

    from mojo_simdjson_amd import _lib, synth

    u = bytearray(synth.workload("utf8", 1 << 20).tobytes())
    arrays = host_arrays(oracle, nm, bytes(u))
    n = len(arrays[0])
    u[int(arrays[0][n // 2])] = ord("x") if arrays[1][n // 2] != ord("x") else ord("y")
    data = bytes(u)
    arrays = host_arrays(oracle, nm, data)
    assert not isinstance(arrays, int)
    n = len(arrays[0])
    dv = dev.device
    d_buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dv)
    d_idx = torch.empty(len(data) + 7, dtype=torch.int32, device=dv)
    d_carry = dev.new_carry()
    d_type = torch.empty(n + 8, dtype=torch.uint8, device=dv)
    d_depth, d_match, d_end = (torch.empty(n + 8, dtype=torch.int32, device=dv) for _ in range(3))
    d_flags = torch.empty(n + 8, dtype=torch.uint8, device=dv)
    d_tok = torch.zeros(24, dtype=torch.uint8, device=dv)
    dev.index(d_buf, d_idx, d_carry)
    rc = dev.lib.msj_stage2_prep_device(dev.ctx, d_buf.data_ptr(), len(data), d_idx.data_ptr(), n, d_type.data_ptr(), d_depth.data_ptr(),
                                        d_match.data_ptr(), d_end.data_ptr(), d_flags.data_ptr(), d_tok.data_ptr(), dev._stream())
    assert rc == 0
    _, d_num = dev.number_values(d_buf, len(data), d_idx, n, d_flags, capacity=0, sync=False)
    d_res = dev.validate(d_buf, len(data), d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_num, sync=False)
    got = _lib.MsjValidateResult.from_buffer_copy(d_res.cpu().numpy().tobytes())  # the one read
    assert dev.fetch(d_carry).count == n
    want = twin_of(twin, data, arrays)
    assert quad(got) == quad(want) and got.code != 0


def test_validate_document_returns_stage1_code(dev):
    assert device_document(dev, b'["abc') == 15  # MSJ_UNCLOSED_STRING
    r = device_document(dev, b'{"a":[1,2,{"b":null}],"c":"\\u00e9"}')
    assert quad(r) == (0, UINT64_MAX, UINT64_MAX, 0) and r.n_escaped == 1
