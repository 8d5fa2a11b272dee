"""msj_stage1 with host pointers through the chunked pipeline (csrc/host_pipe.cpp), at its 16 MiB chunk borders.

The smallest inputs that have a border are two and three chunks, 32 to 48 MiB (one sequence needs four: 64 MiB).  Every result is
compared with the oracle -- index array, count, trailer, return code, UTF-8 verdict -- and, where the reference says
nothing (a capacity below the count), with the same call through plain staging, word for word.  No test here makes the
device fail: failure injection lives on the fake device of tests/cpp/host_pipe_sanitize.cpp only."""
import contextlib
import ctypes

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

C = 16 << 20           # HostPipe::kChunk
SENTINEL = 0xDEADBEEF
GUARD = 64             # words behind the capacity that no call may touch
N_NOT_SET = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    from mojo_simdjson_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def docs():
    """Two complete documents of just under one chunk each: multi-byte UTF-8 with escapes, and minified ASCII."""
    from mojo_simdjson_amd import synth

    u, m = synth.workload("utf8", 15 << 20), synth.workload("minified", 15 << 20)
    for d in (u, m):
        assert (14 << 20) < d.size < C - (1 << 16)
    return u, m


@contextlib.contextmanager
def pipeline_from(lib, min_bytes):
    """Inputs from min_bytes on take the pipeline; the default (64 MiB) again afterwards, whatever happens."""
    assert lib.msj_debug_set_pipeline_min_bytes(None, min_bytes) == 0
    try:
        yield
    finally:
        lib.msj_debug_set_pipeline_min_bytes(None, 0)


def padded_front(parts, total):
    """The parts behind as many spaces as make `total` bytes: the input ends on the last part's last byte."""
    used = sum(len(p) for p in parts)
    assert used <= total
    out = np.empty(total, dtype=np.uint8)
    out[: total - used] = 0x20
    at = total - used
    for p in parts:
        out[at: at + len(p)] = np.frombuffer(bytes(p), dtype=np.uint8) if isinstance(p, (bytes, bytearray)) else p
        at += len(p)
    return out


def across_border(docs, pre, post):
    """Two chunks: a document, then `pre` ending on the last byte of chunk 0, `post` from the first byte of chunk 1 on, then
    the other document."""
    u, m = docs
    left = padded_front([u, b" ", pre], C)
    out = np.concatenate([left, np.frombuffer(post + b" ", dtype=np.uint8), m])
    assert C < out.size <= 2 * C and bytes(out[C - len(pre): C + len(post)]) == pre + post
    return out


def stage1(lib, data, cap=None, arena=None, offset=0):
    """-> (rc, n, verdict, array): array[:cap] is the caller's index array, array[cap:] the guard behind it."""
    cap = data.size + 3 if cap is None else cap
    if arena is None:
        arena = np.empty(offset + cap + GUARD, dtype=np.uint32)
    view = arena[offset: offset + cap + GUARD]
    view[:] = SENTINEL
    n, verdict = ctypes.c_uint64(N_NOT_SET), ctypes.c_int32(-1)
    rc = lib.msj_stage1(ctypes.c_void_p(data.ctypes.data), data.size, ctypes.c_void_p(view.ctypes.data), cap,
                        ctypes.byref(n), ctypes.byref(verdict), 0)
    return rc, n.value, verdict.value, view


def check_against_oracle(lib, oracle, data, where, arena=None, offset=0):
    raw = data.tobytes()
    code, n, want = helpers.run_oracle(oracle.msj_oracle_stage1, raw)
    rc, got_n, verdict, arr = stage1(lib, data, arena=arena, offset=offset)
    assert rc == code, f"{where}: code {rc}, oracle {code}"
    assert verdict == oracle.msj_oracle_utf8(raw, len(raw)), f"{where}: UTF-8 verdict {verdict}"
    if n is None:
        assert got_n == N_NOT_SET, f"{where}: n set to {got_n} though the reference returns before it sets it"
        return code, None
    assert got_n == n, f"{where}: n {got_n}, oracle {n}"
    if not np.array_equal(arr[: n + 3], want):
        bad = int(np.argmax(arr[: n + 3] != want))
        raise AssertionError(f"{where}: index {bad} of {n} + 3 is {arr[bad]}, oracle {want[bad]}")
    assert (arr[n + 3:] == SENTINEL).all(), f"{where}: a word behind the trailer was written"
    return code, n


def test_lengths_one_byte_either_side_of_a_chunk(lib, oracle, docs):
    """2 * C - 1, 2 * C and 2 * C + 1 bytes: the last chunk one byte short, exactly full, and a third chunk of one
    byte.  The border lies inside the first document, the input ends on the second one's closing brace."""
    u, m = docs
    with pipeline_from(lib, 24 << 20):
        for total in (2 * C - 1, 2 * C, 2 * C + 1):
            data = padded_front([u, b" ", m], total)
            assert data[-1] == ord("}") and data[C - 1] != 0x20 and data[C] != 0x20
            code, n = check_against_oracle(lib, oracle, data, f"{total} bytes")
            assert code == 0 and n > 1 << 20


def test_backslash_runs_that_end_on_the_last_byte_of_a_chunk(lib, oracle, docs):
    """A run of backslashes ends on the last byte of chunk 0 and a quote opens chunk 1: behind an odd run the quote is
    escaped and the string goes on, behind an even run it closes the string."""
    with pipeline_from(lib, 24 << 20):
        counts = {}
        for run in (1, 2, 7, 8):
            post = b'" , 1 ] ," , 2 ] ' if run % 2 else b'" , 1 ] , 2 ] '  # (either way no string is left open)
            data = across_border(docs, b'["abc' + b"\\" * run, post)
            code, counts[run] = check_against_oracle(lib, oracle, data, f"{run} backslashes before the border")
            assert code == 0
        # (the escaped quote keeps ` , 1 ] ,` inside the string: fewer structurals)
        assert counts[1] == counts[7] and counts[2] == counts[8] and counts[1] != counts[2]


def test_string_and_scalars_across_the_border(lib, oracle, docs):
    """A string open across the border; a scalar that ends exactly at the border (the next chunk starts on the comma, and
    on a fresh scalar); a scalar that goes on across it (no second structural)."""
    with pipeline_from(lib, 24 << 20):
        n = {}
        for name, pre, post in (("string", b'["a string, that [ does ] not: ', b'end, here" , 5 ] '),
                                ("scalar then comma", b"[ 12345", b", 6789 ] "),
                                ("scalar then scalar", b"[ true", b"false ] "),
                                ("scalar then space", b"[ 12345", b" 6789 ] "),
                                ("scalar goes on", b"[ 123", b"45 , 6789 ] ")):
            code, n[name] = check_against_oracle(lib, oracle, across_border(docs, pre, post), name)
            assert code == 0
        # [ 12345 , 6789 ] either way with the comma; one structural fewer without it; `truefalse` is one scalar
        assert n["scalar then comma"] == n["scalar goes on"] == n["scalar then space"] + 1 == n["scalar then scalar"] + 2


def test_four_byte_utf8_sequence_split_by_the_border(lib, oracle, docs):
    """U+1F600 inside a string, split behind its first, second and third byte: valid, and then with the byte that opens
    chunk 1 no continuation byte."""
    seq = "\U0001F600".encode()
    with pipeline_from(lib, 24 << 20):
        for split in (1, 2, 3):
            for broken in (False, True):
                tail = seq[split:]
                if broken:
                    tail = b"A" + tail[1:]
                data = across_border(docs, b'["x' + seq[:split], tail + b'y" , 1 ] ')
                raw = data.tobytes()
                assert oracle.msj_oracle_utf8(raw, len(raw)) == (11 if broken else 0)
                code, _ = check_against_oracle(lib, oracle, data, f"split after {split} bytes, broken={broken}")
                assert code == 0  # (the verdict is reported beside the code)


def test_capacity_round_the_count_matches_plain_staging(lib, oracle, docs):
    """idx_capacity of n + 3, n + 2, n and n - 1 on a two-chunk input: return code, count, verdict and every word up to
    the capacity are those of the same call through plain staging, and no word behind the capacity is written."""
    u, m = docs
    data = padded_front([u, b" ", m], 2 * C)
    raw = data.tobytes()
    code, n, want = helpers.run_oracle(oracle.msj_oracle_stage1, raw)
    assert code == 0
    arena = np.empty(n + 3 + GUARD, dtype=np.uint32)
    for cap in (n + 3, n + 2, n, n - 1):
        with pipeline_from(lib, 24 << 20):
            rc, got_n, verdict, arr = stage1(lib, data, cap=cap, arena=arena)
            piped = (rc, got_n, verdict, arr[:cap].copy())
            assert (arr[cap:] == SENTINEL).all(), f"capacity {cap - n:+d}: the pipeline wrote behind the capacity"
        rc, got_n, verdict, arr = stage1(lib, data, cap=cap, arena=arena)  # 32 MiB: below the default threshold
        assert (arr[cap:] == SENTINEL).all(), f"capacity {cap - n:+d}: plain staging wrote behind the capacity"
        assert piped[:3] == (rc, got_n, verdict), f"capacity n{cap - n:+d}: pipeline {piped[:3]}, plain {(rc, got_n, verdict)}"
        assert np.array_equal(piped[3], arr[:cap]), f"capacity n{cap - n:+d}: the arrays differ"
        # and both are right: everything with room for the trailer, else CAPACITY over the clipped indices
        if cap >= n + 3:
            assert (rc, got_n, verdict) == (0, n, 0) and np.array_equal(arr[: n + 3], want)
        else:
            assert (rc, got_n, verdict) == (1, N_NOT_SET, 0)
            assert np.array_equal(arr[: min(n, cap)], want[: min(n, cap)]) and (arr[min(n, cap): cap] == SENTINEL).all()


def test_one_context_three_chunks_then_two_then_four(lib, oracle, docs):
    """The default context across calls of three, two and four chunks: the smaller call runs over the larger one's
    carries and events, the larger one regrows them.  Input and index array are registered for the middle call only
    (the index array as a view inside its registered range)."""
    u, m = docs
    three = padded_front([u, b" ", m, b" ", u], 3 * C - 4321)
    two = padded_front([m, b" ", u], 2 * C - 77)
    four = padded_front([u, b" ", m, b" ", u, b" ", m], 4 * C - 12345)
    arena = np.empty(512 + two.size + 3 + GUARD, dtype=np.uint32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    with pipeline_from(lib, 24 << 20):
        assert check_against_oracle(lib, oracle, three, "three chunks")[0] == 0
        assert lib.msj_host_register(None, vp(arena), arena.nbytes) == 0
        try:
            assert lib.msj_host_register(None, vp(two), two.nbytes) == 0
            try:
                assert check_against_oracle(lib, oracle, two, "two chunks, registered", arena=arena, offset=512)[0] == 0
            finally:
                assert lib.msj_host_unregister(None, vp(two)) == 0
        finally:
            assert lib.msj_host_unregister(None, vp(arena)) == 0
        assert check_against_oracle(lib, oracle, four, "four chunks")[0] == 0
