"""Number values for stage 2 (msj_number_values_device, csrc/numbers_kernel.hip) on the device.

Stage 1, then the spans, then the number call, all on the GPU through the C ABI.  Expected values come from Python
(json.loads, int(), float() with the definition's int64 and finite-range rules: tests/test_number_math.expected) and from
the host twin of the same arithmetic (tests/number_math_host.cpp).  DERIVED like the token arrays: the definition is
include/msj_stage1.h's, the reference's own parse_number cannot run here.
The readers behind the arithmetic (the lane window, the wave steps) at every phase: tests/test_number_phases.py.
"""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from tests import helpers
from tests import test_number_math as tnm

UINT64_MAX = (1 << 64) - 1
ERRORS = (tnm.ERR_SYNTAX, tnm.ERR_RANGE)


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
    return tnm.load_twin()


def _on_device(dev, data, behind=b"", pairs=False):
    """stage 1 + spans on the device: (d_buf, d_idx, n, d_flags).  behind: bytes that lie in the device tensor past the
    buffer's end (every call gets len(data)); pairs: the spans of msj_stage2_prep_pairs_device instead of the span call's,
    nothing waited for in between."""
    import torch

    d_buf = torch.from_numpy(np.frombuffer(data + behind, dtype=np.uint8).copy()).to(dev.device)[:len(data)]
    d_idx = torch.empty(len(data) + 3 + 4, dtype=torch.int32, device=dev.device)
    d_res = dev.new_carry()
    dev.index(d_buf, d_idx, d_res)
    r = dev.fetch(d_res)
    assert r.code == 0, r.code
    n = int(r.count)
    if pairs:
        d_flags = dev.stage2_prep_pairs(d_buf, len(data), d_idx, n, spans=True)[4][:n]
    else:
        _, d_flags = dev.token_spans(d_buf, len(data), d_idx, n)
    return d_buf, d_idx, n, d_flags


def _records(d_numbers, count):
    rec = d_numbers[:count].cpu().numpy()
    bits = rec[:, 0].view(np.uint64)
    hi = rec[:, 1].view(np.uint64)
    return bits, (hi & 0xFFFFFFFF).astype(np.uint32), (hi >> np.uint64(32)).astype(np.uint32)


def _twin_values(twin, data, starts, length=None):
    """length: the buffer's len where `data` goes on behind it"""
    starts = np.ascontiguousarray(starts, dtype=np.uint64)
    bits = np.zeros(starts.size, dtype=np.uint64)
    kinds = np.zeros(starts.size, dtype=np.uint32)
    paths = np.zeros(3, dtype=np.uint64)
    twin.nm_convert_batch(data, len(data) if length is None else length, starts.ctypes.data, starts.size, bits.ctypes.data,
                          kinds.ctypes.data, paths.ctypes.data)
    return bits, kinds, paths


def _check_call(dev, twin, data, where, python_sample=None, seed=0, behind=b"", pairs=False, seen=None):
    """Every record against the twin, the counts against a host scan of the flags and the twin's paths, (a sample of) the
    records against Python.  -> (bits, tokens, kinds, result).  behind, pairs: _on_device's; seen: a dict that receives
    what the call saw (idx, flags, the number tokens, the buffer's address)."""
    d_buf, d_idx, n, d_flags = _on_device(dev, data, behind, pairs)
    d_numbers, res = dev.number_values(d_buf, len(data), d_idx, n, d_flags)
    idx = d_idx[:n].cpu().numpy().view(np.uint32)
    flags = d_flags[:n].cpu().numpy()
    num_tok = np.nonzero(flags & 4)[0]
    assert res.n_numbers == num_tok.size, where
    bits, tokens, kinds = _records(d_numbers, num_tok.size)
    assert np.array_equal(tokens, num_tok.astype(np.uint32)), where
    if seen is not None:
        seen.update(idx=idx, flags=flags, num_tok=num_tok, address=d_buf.data_ptr())
    wb, wk, paths = _twin_values(twin, data + behind, idx[num_tok], len(data))
    bad = np.nonzero((wb != bits) | (wk != kinds))[0]
    assert bad.size == 0, (where, [(int(tokens[i]), data[idx[tokens[i]]:idx[tokens[i]] + 40]) for i in bad[:3]])
    err = np.isin(kinds, ERRORS)
    assert res.n_errors == int(err.sum()), where
    assert res.first_error == (int(tokens[np.argmax(err)]) if err.any() else UINT64_MAX), where
    assert res.n_slow == int(paths[2]), where  # the exact path: the same numbers on the device as in the twin
    # flagged MSJ_SPAN_BAD: a syntax error
    assert (kinds[(flags[num_tok] & 32) != 0] == tnm.ERR_SYNTAX).all(), where
    pick = range(num_tok.size)
    if python_sample is not None and num_tok.size > python_sample:
        pick = sorted(random.Random(seed).sample(range(num_tok.size), python_sample))
    for i in pick:
        assert (int(kinds[i]), int(bits[i])) == tnm.expected(data, int(idx[num_tok[i]])), (where, i)
    return bits, tokens, kinds, res


def _json_numbers(v, out):
    if isinstance(v, bool) or v is None or isinstance(v, str):
        return out
    if isinstance(v, (int, float)):
        out.append(v)
    elif isinstance(v, dict):
        for x in v.values():
            _json_numbers(x, out)
    else:
        for x in v:
            _json_numbers(x, out)
    return out


@pytest.mark.gpu
def test_fixtures_equal_json_loads(dev, twin):
    """The reference fixtures that hold numbers: the records, in token order, are the numbers json.loads yields in
    document order."""
    import struct

    names = [f for f in os.listdir(os.path.join(helpers.GOLDEN, "valid"))
             if f.startswith(("root_int_", "root_float_")) or f in ("simple_floats.json", "simple_json.json")]
    assert len(names) >= 6
    for name in sorted(names):
        js, _ = helpers.read_fixture(os.path.join(helpers.GOLDEN, "valid", name))
        bits, tokens, kinds, res = _check_call(dev, twin, js, name)
        want = _json_numbers(json.loads(js), [])
        assert len(want) == res.n_numbers > 0, name
        assert res.n_errors == 0 and res.first_error == UINT64_MAX
        for v, b, k in zip(want, bits.tolist(), kinds.tolist()):
            if isinstance(v, int):
                assert (k, b) == (tnm.INT64, v & UINT64_MAX), (name, v)
            else:
                assert (k, b) == (tnm.DOUBLE, struct.unpack("<Q", struct.pack("<d", v))[0]), (name, v)


def _array(texts, sep=b","):
    return b"[" + sep.join(texts) + b"]"


@pytest.mark.gpu
def test_cpu_corpus_on_the_device(dev, twin):
    """The corpus of tests/test_number_math.py as JSON arrays: bit-equal to Python, long numbers (over 1024 characters:
    the MSJ_SPAN_LONG wave path) and a 1 MiB one included."""
    rng = np.random.default_rng(12)
    raw = rng.integers(0, 0x7FF0000000000000, 50_000, dtype=np.uint64) | (rng.integers(0, 2, 50_000, dtype=np.uint64) << np.uint64(63))
    texts = []
    for v in raw.view(np.float64).tolist():
        texts += [repr(v).encode(), b"%.17e" % v, b"%.25e" % v, b"%.40g" % v]
    r = random.Random(5)
    texts += [str(r.randrange(-(1 << 63), 1 << 63)).encode() for _ in range(20_000)]
    for c in (1 << 53, 1 << 63, -(1 << 63), 10 ** 19, -(10 ** 19)):
        texts += [str(c + d).encode() for d in (-1, 0, 1)]
    _check_call(dev, twin, _array(texts), "random doubles and integers")
    _, _, _, res = _check_call(dev, twin, _array(tnm._halfway_texts(random.Random(7), 600)), "halfway points")
    assert res.n_slow > 0
    long_texts = tnm.boundary_texts()
    assert max(len(t) for t in long_texts) > 1024
    _, _, _, res = _check_call(dev, twin, _array(long_texts, b", "), "boundaries and long numbers")
    assert res.n_slow > 0
    # a 1 MiB number: integer (range error), float, float that underflows; inside an object and at the end of the buffer
    d = "".join(r.choice("0123456789") for _ in range(1 << 20)).encode()
    big = [b"7" + d, b"3." + d, b"-0." + d + b"e-400", b"1" + d[:2000] + b"e-2005"]
    _check_call(dev, twin, b'{"a":' + big[0] + b',"b":[' + big[1] + b"," + big[2] + b"]," + b'"c":' + big[3] + b"}", "1 MiB numbers")
    _check_call(dev, twin, b"[1, 2.5, " + big[1], "1 MiB number at the end of the buffer")
    # the syntax corpus, and the bad string of test_tokens.test_spans_follow_the_reference_scans
    _, _, kinds, res = _check_call(dev, twin, _array([t for t in tnm.SYNTAX if t[:1] in b"-0123456789"], b" , "), "syntax")
    assert set(kinds.tolist()) == {tnm.ERR_SYNTAX} and res.n_errors == res.n_numbers
    _check_call(dev, twin, b'[12a,-,--1,1+2,1.5x,1e5,-0.5E-3,0x10,1.,12 ,3\t,4\n,5:6,7"a",1.5"b" ,9]', "bad")


@pytest.mark.gpu
def test_every_number_takes_the_fallback(dev, twin):
    """64 MiB of numbers that all need the exact path: correct, and n_slow counts every one of them (more than the
    fallback list holds: the overflow sweep resolves them)."""
    import torch

    texts = tnm.fallback_texts(random.Random(21), 4000)
    unit = b",".join(texts) + b","
    reps = (64 << 20) // len(unit)
    data = b"[" + unit * reps + b"0.5]"
    d_buf, d_idx, n, d_flags = _on_device(dev, data)
    d_numbers, res = dev.number_values(d_buf, len(data), d_idx, n, d_flags)
    count = len(texts) * reps + 1
    assert res.n_numbers == count and res.n_errors == 0 and res.first_error == UINT64_MAX
    assert res.n_slow == count - 1  # 0.5: the fast path
    wb, wk, paths = _twin_values(twin, b"[" + unit + b"]", 1 + np.cumsum([0] + [len(t) + 1 for t in texts[:-1]]))
    assert paths.tolist() == [0, 0, len(texts)]
    for i in range(0, len(texts), 97):
        assert (int(wk[i]), int(wb[i])) == tnm.expected(texts[i] + b",")
    rec = d_numbers[: count - 1].view(reps, len(texts), 2)
    want = torch.from_numpy(wb.view(np.int64)).to(dev.device)
    assert torch.equal(rec[:, :, 0], want.expand(reps, -1))
    assert bool(((rec[:, :, 1] >> 32) == tnm.DOUBLE).all())


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["minified", "utf8", "pretty4"])
def test_workloads_1mib(dev, twin, workload):
    from mojo_simdjson_amd import synth

    u = synth.workload(workload, 1 << 20).tobytes()
    _, _, _, res = _check_call(dev, twin, u, workload, python_sample=100_000)
    assert res.n_numbers > 1000


@pytest.mark.gpu
def test_minified_1gib(dev, twin):
    """1 GiB (a 64 MiB unit 16 times; every unit a complete document): every record equals the twin's for its unit, a
    seeded sample of 100 000 equals Python."""
    import torch

    from mojo_simdjson_amd import synth

    u = synth.workload("minified", 64 << 20)
    ub = u.tobytes()
    reps = 16
    d_buf = torch.from_numpy(u).to(dev.device).repeat(reps)
    d_idx = torch.empty(d_buf.numel() // 2, dtype=torch.int32, device=dev.device)
    d_res = dev.new_carry()
    dev.index(d_buf, d_idx, d_res)
    n = int(dev.fetch(d_res).count)
    assert n % reps == 0
    nu = n // reps
    _, d_flags = dev.token_spans(d_buf, d_buf.numel(), d_idx, n)
    d_numbers, res = dev.number_values(d_buf, d_buf.numel(), d_idx, n, d_flags)
    idx_u = d_idx[:nu].cpu().numpy().view(np.uint32)
    flags_u = d_flags[:nu].cpu().numpy()
    tok_u = np.nonzero(flags_u & 4)[0]
    assert res.n_numbers == tok_u.size * reps
    err = np.zeros(0)
    wb, wk, _ = _twin_values(twin, ub, idx_u[tok_u])
    err = np.isin(wk, ERRORS)
    assert res.n_errors == int(err.sum()) * reps
    assert res.first_error == (int(tok_u[np.argmax(err)]) if err.any() else UINT64_MAX)
    rec = d_numbers[: tok_u.size * reps].view(reps, tok_u.size, 2)
    assert torch.equal(rec[:, :, 0], torch.from_numpy(wb.view(np.int64)).to(dev.device).expand(reps, -1))
    tok = torch.from_numpy(tok_u.astype(np.int64)).to(dev.device)[None, :] + torch.arange(reps, device=dev.device)[:, None] * nu
    want_hi = tok | (torch.from_numpy(wk.astype(np.int64)).to(dev.device)[None, :] << 32)
    assert torch.equal(rec[:, :, 1], want_hi)
    r = random.Random(3)
    for i in r.sample(range(tok_u.size), 100_000):
        assert (int(wk[i]), int(wb[i])) == tnm.expected(ub, int(idx_u[tok_u[i]])), i


@pytest.mark.gpu
def test_capacity_clips_the_list_not_the_counts(dev, twin):
    from mojo_simdjson_amd import synth

    u = synth.workload("minified", 1 << 20).tobytes() + b" [1e400, 2]"
    d_buf, d_idx, n, d_flags = _on_device(dev, u)
    full, rf = dev.number_values(d_buf, len(u), d_idx, n, d_flags)
    cap = rf.n_numbers // 3
    part, rp = dev.number_values(d_buf, len(u), d_idx, n, d_flags, capacity=cap)
    assert (rp.n_numbers, rp.n_errors, rp.first_error, rp.n_slow) == (rf.n_numbers, rf.n_errors, rf.first_error, rf.n_slow)
    assert rf.n_errors >= 1
    import torch

    assert torch.equal(part[:cap], full[:cap])


@pytest.mark.gpu
def test_empty_call_and_misaligned_records(dev):
    import torch

    d_buf = torch.zeros(16, dtype=torch.uint8, device=dev.device)
    d_idx = torch.zeros(16, dtype=torch.int32, device=dev.device)
    d_flags = torch.zeros(16, dtype=torch.uint8, device=dev.device)
    _, res = dev.number_values(d_buf, 16, d_idx, 0, d_flags)
    assert (res.n_numbers, res.n_errors, res.first_error, res.n_slow) == (0, 0, UINT64_MAX, 0)
    # a misaligned d_numbers: MSJ_ERR_BAD_ARGUMENT, nothing launched (the result keeps its pattern)
    d_flags[0] = 4
    d_res = torch.full((32,), 0x5A, dtype=torch.uint8, device=dev.device)
    d_num = torch.zeros(64, dtype=torch.uint8, device=dev.device)
    p = ctypes.c_void_p
    rc = dev.lib.msj_number_values_device(dev.ctx, p(d_buf.data_ptr()), 16, p(d_idx.data_ptr()), 1, p(d_flags.data_ptr()),
                                          p(d_num.data_ptr() + 8), 2, p(d_res.data_ptr()), dev._stream())
    assert rc == -1
    torch.cuda.synchronize()
    assert bool((d_res == 0x5A).all()) and bool((d_num == 0).all())
    rc = dev.lib.msj_number_values_device(dev.ctx, p(d_buf.data_ptr()), 16, p(d_idx.data_ptr() + 4), 1, p(d_flags.data_ptr()),
                                          p(d_num.data_ptr()), 2, p(d_res.data_ptr()), dev._stream())
    assert rc == -1


@pytest.mark.gpu
def test_chains_behind_prep_pairs(dev):
    """Behind msj_stage2_prep_pairs_device in one stream, no synchronisation in between: the same records."""
    import torch

    from mojo_simdjson_amd import synth

    u = synth.workload("minified", 4 << 20).tobytes()
    d_buf, d_idx, n, d_flags = _on_device(dev, u)
    want, rw = dev.number_values(d_buf, len(u), d_idx, n, d_flags)
    torch.cuda.synchronize()
    _, _, _, _, d_flags2, _ = dev.stage2_prep_pairs(d_buf, len(u), d_idx, n, spans=True)
    got, d_res = dev.number_values(d_buf, len(u), d_idx, n, d_flags2, sync=False)
    from mojo_simdjson_amd import _lib

    rg = _lib.MsjNumbersResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
    assert (rg.n_numbers, rg.n_errors, rg.first_error, rg.n_slow) == (rw.n_numbers, rw.n_errors, rw.first_error, rw.n_slow)
    assert torch.equal(got[: rw.n_numbers], want[: rw.n_numbers])
