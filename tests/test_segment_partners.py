"""Bracket partners over a whole shard (msj_stage2_prep_segments with d_match, include/msj_stage1.h).

Every segment pairs what closes inside it and leaves the rest in a residual list indexed by depth; a stitch behind the
last segment walks back over the segments for every closing bracket.  A wrong partner is not an error anywhere else, so
every token's partner is compared here with the definition: the stack of start_container / end_container on the
shard's whole token stream (helpers.oracle_match), mapped to the shard's output positions.  The definition of the clip
(include/msj_stage1.h: the residual lists hold MSJ_RESID_CAP levels from each segment's minimum running depth up) is
stated in _expected below, and the header's promise -- every container less than 65 536 levels above the shard's
minimum running depth is stitched -- is checked on its own.

The cases are built on the host from their token stream (stage 1's definition, the C oracle): segment borders on the
16-byte grid, blanks in front of a bracket to put a border exactly before or behind it."""
import ctypes
import functools

import numpy as np
import pytest

from tests import helpers

CAP = 65536  # MSJ_RESID_CAP: levels per residual list
NONE = 0xFFFFFFFF
MSJ_CAPACITY = 1
OPEN, CLOSE = b"[{", b"]}"


# ---- the cases: bytes, the shard's first byte, segment borders -------------------------------------------------------
class Doc:
    """A stream built piece by piece, with segment borders placed at exact token edges."""

    def __init__(self):
        self.parts, self.len, self.borders = [], 0, []

    def add(self, b):
        self.parts.append(b)
        self.len += len(b)
        return self

    def _pad(self, k):  # blanks until the length is k modulo 16
        return self.add(b" " * ((k - self.len) % 16))

    def border(self):
        """A border in front of whatever comes next."""
        self._pad(0)
        if self.len and (not self.borders or self.borders[-1] != self.len):
            self.borders.append(self.len)
        return self

    def then_border(self, tok):
        """tok (one byte) as the last byte in front of a border."""
        self._pad(15).add(tok)
        self.borders.append(self.len)
        return self

    def bytes(self):
        return b"".join(self.parts)


class Case:
    def __init__(self, name, data, borders, prefix=0):
        assert prefix % 16 == 0 and all(b % 16 == 0 and prefix < b < len(data) for b in borders), name
        self.name, self.data, self.prefix = name, bytes(data), prefix
        self.borders = sorted(set(borders))


def grid_borders(prefix, length, seg):
    return list(range(prefix + seg, length, seg))


_FILLERS = [b"1,", b'"ab",', b"true,", b'"[[{]]}",', b"-2.5e3,", b"null,", b'{"k":[1,2]},', b'"x\\"]",', b"[],"]


def random_profile(seed, kind, size):
    """A seeded depth profile with scalars, strings (some full of brackets) and small containers between the brackets:
    'ramp' climbs to ~20 000 levels and back, 'saw' is a sawtooth, 'plateau' climbs and stays, 'below' starts with
    stray closing brackets (below the depth the shard starts at) and climbs from there."""
    rng = np.random.default_rng(seed)
    out, stack, depth = [], [], 0
    n = 0

    def step_to(target, fill):
        nonlocal depth, n
        k = abs(target - depth)
        fills = (rng.random(k) < fill).tolist()
        picks = rng.integers(0, len(_FILLERS), k).tolist()
        kinds = rng.integers(0, 2, k).tolist()
        for j in range(k):
            if target > depth:
                stack.append(kinds[j])
                out.append(b"[{"[kinds[j]:kinds[j] + 1])
            else:  # the bracket that closes the innermost container; a stray ']' below the start
                out.append(b"]}"[stack[-1]:stack[-1] + 1] if stack else b"]")
                if stack:
                    stack.pop()
            depth += 1 if target > depth else -1
            n += 1
            if fills[j]:
                out.append(_FILLERS[picks[j]])
                n += len(_FILLERS[picks[j]])

    if kind == "below":
        step_to(-int(rng.integers(100, 3000)), 0.2)
    while n < size:
        if kind == "ramp":
            step_to(int(rng.integers(15000, 20000)), 0.3)
            step_to(int(rng.integers(-50, 50)) if depth < 0 else 0, 0.3)
        elif kind == "saw":
            step_to(depth + int(rng.integers(50, 3000)), 0.5)
            step_to(max(depth - int(rng.integers(50, 3000)), -200), 0.5)
        elif kind == "plateau":
            step_to(int(rng.integers(500, 5000)), 0.2)
            k = int(rng.integers(1000, 20000))
            out.append(b"7," * k)
            n += 2 * k
            step_to(int(rng.integers(0, 200)), 0.2)
        else:  # below
            step_to(depth + int(rng.integers(100, 4000)), 0.4)
            step_to(depth - int(rng.integers(50, 2000)), 0.4)
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def random_cases():
    cases = []
    # (bytes at least: a profile ends with its cycle; 2 .. 32 segments each)
    for k, (kind, seg, size) in enumerate([("ramp", 4096, 1), ("saw", 4096, 100000), ("below", 4096, 30000), ("ramp", 8192, 150000),
                                           ("plateau", 8192, 200000), ("saw", 65536, 1900000), ("below", 65536, 300000),
                                           ("ramp", 1 << 20, 1300000), ("saw", 1 << 20, 2300000)]):
        data = random_profile(100 + k, kind, size)
        cases.append(Case(f"random {kind}, {seg}-byte segments", data, grid_borders(0, len(data), seg)))
    return cases


@functools.lru_cache(maxsize=None)
def placement_cases():
    """Every way a partner can lie, borders at the edges of tokens."""
    cases = []
    d = Doc().add(b"[1,[2,3],")  # a partner in the same segment
    d.then_border(b"[").add(b"4,").then_border(b"]")  # borders right behind brackets: the partner in the segment in front
    d.add(b",[5").border().add(b"]").border()  # a border right in front of a closing bracket
    d.add(b",{").add(b'"a":[' * 50).border()  # 50 + 1 levels opened here ...
    d.add(b"1,2").border().add(b"3,[[[]]]").border()  # ... two segments that never come down to them ...
    d.add(b"]" * 20).add(b"[" * 20).border()  # ... one that closes 20 of them and opens them again ...
    d.add(b"]" * 50 + b"}").border()  # ... and their closing brackets: 30 levels several segments back, 20 one back
    d.add(b",[").border().add(b"[").border().add(b"]").border().add(b"]]")  # one bracket per segment; the root closes
    d.add(b"]]").border().add(b"[[[")  # partners in front of the shard; never closed
    cases.append(Case("placements", d.bytes(), d.borders))

    d = Doc().add(b'["')  # a string full of brackets over many borders, one segment with no token at all
    for _ in range(3):
        d.add(b"[[[{" * 300).border().add(b"]]}]" * 400)
    d.add(b'",').border()
    d.add(b'"' + b"]" * 5000 + b'"]').border().add(b'[1]')
    cases.append(Case("borders inside strings, an empty segment", d.bytes(), d.borders))

    body = b"[" + b"1," * 3000 + b'"' + b"x" * 9000 + b'",[' + b"2," * 3000 + b"]]"
    cases.append(Case("a token-less segment between the ends of a container", body, grid_borders(0, len(body), 4096)))

    closers = b"]" * 9000
    cases.append(Case("only closing brackets", closers, grid_borders(0, len(closers), 4096)))
    openers = b"{" * 9000
    cases.append(Case("only opening brackets", openers, grid_borders(0, len(openers), 4096)))
    # the same with the stream in front: the closing brackets pair with nothing inside the shard
    pre = b"[" * 9008
    cases.append(Case("only closing brackets, d_prev deep", pre + closers, grid_borders(len(pre), len(pre + closers), 4096), prefix=len(pre)))
    return cases


@functools.lru_cache(maxsize=None)
def prev_cases():
    """A shard that does not start its stream: depth 37 in front of it, and -5."""
    cases = []
    shard = random_profile(7, "saw", 60000)
    for name, pre in (("d_prev at depth 37", b'{"a":[' * 18 + b"[1,"), ("d_prev at depth -5", b"[]]]]]]")):
        pre += b" " * (-len(pre) % 16)
        body = b"]" * 60 + shard + b"[" * 45  # goes below the shard's start depth first
        data = pre + body
        cases.append(Case(name, data, grid_borders(len(pre), len(data), 8192), prefix=len(pre)))
    return cases


@functools.lru_cache(maxsize=None)
def clip_cases():
    """Nesting over MSJ_RESID_CAP levels at a border (the lists keep the levels nearest each segment's minimum)."""
    cases = []
    deep = b"[" * 70000 + b"]" * 70000
    cases.append(Case("70 000 deep, 69 632-byte segments", deep, grid_borders(0, len(deep), 69632)))
    run = b"[" * 150000 + b"]" * 150000  # an opener run over two borders
    cases.append(Case("150 000 deep, 69 632-byte segments", run, grid_borders(0, len(run), 69632)))
    d = Doc().add(b"[" * 100).border().add(b"]" * 70000).add(b"[" * 5)  # > 65 536 stray closers behind a border
    cases.append(Case("70 000 stray closing brackets behind a border", d.bytes(), d.borders))
    return cases


# ---- the definition --------------------------------------------------------------------------------------------------
_ORACLE = []


def _index(data):
    """Stage 1's structural indices (the C oracle)."""
    if not _ORACLE:
        _ORACLE.append(helpers.load_oracle())
    _, n, idx = helpers.run_oracle(_ORACLE[0].msj_oracle_stage1, data)
    assert n is not None
    return idx[:n].astype(np.int64)


class Expected:
    pass


def _round8(n):
    return (n + 7) // 8 * 8


def _expected(case, idx=None):
    """What msj_stage2_prep_segments must leave for the case: the segment table, the shard's types / depths / results,
    and every token's partner as a position in the shard's output arrays."""
    e = Expected()
    idx = _index(case.data) if idx is None else idx
    typ, dep, _ = helpers.oracle_tokens(case.data, idx)
    partner = helpers.oracle_match(typ).astype(np.int64)
    delta = np.isin(typ, list(OPEN)).astype(np.int64) - np.isin(typ, list(CLOSE)).astype(np.int64)
    after = dep.astype(np.int64) + (delta > 0)  # the running depth behind each token
    p = int(np.searchsorted(idx, case.prefix))  # tokens in front of the shard
    bases = [case.prefix] + case.borders
    ends = case.borders + [len(case.data)]
    first = [int(np.searchsorted(idx, b)) for b in bases] + [idx.size]
    e.segs, e.offs, off = [], [], 0
    for s in range(len(bases)):
        cnt = first[s + 1] - first[s]
        e.segs.append((bases[s] - case.prefix, ends[s] - bases[s], first[s] - p, cnt))
        e.offs.append(off)
        off += _round8(cnt)
    e.total = off
    e.idx_rel = np.concatenate([idx[first[s]:first[s + 1]] - bases[s] for s in range(len(bases))])
    e.prefix_n, e.prefix_final = p, int(after[p - 1]) if p else 0
    e.prefix_result = (p, e.prefix_final, int(after[:p].min()) if p else 0, int(after[:p].max()) if p else 0,
                       int((delta[:p] > 0).sum()))
    n = idx.size - p
    e.typ, e.dep = typ[p:], dep[p:]
    seg = np.repeat(np.arange(len(bases)), np.diff(first))
    ib = np.array([sg[2] for sg in e.segs], dtype=np.int64)
    pos = np.array(e.offs, dtype=np.int64)[seg] + np.arange(n) - ib[seg]
    # per segment: the depth in front of it and its minimum running depth (its start depth included)
    start, low, e.results = [], [], []
    d = e.prefix_final
    for s in range(len(bases)):
        a = after[first[s]:first[s + 1]]
        start.append(d)
        low.append(min([d] + ([int(a.min())] if a.size else [])))
        d = int(a[-1]) if a.size else d
        so_far = after[:first[s + 1]]
        e.results.append((first[s + 1] - first[s], d, int(so_far.min()) if so_far.size else 0,
                          int(so_far.max()) if so_far.size else 0, int((delta[first[s]:first[s + 1]] > 0).sum())))
    e.start, e.low = start, low
    # partners: in the shard or not at all; across a border, stitched while the level lies less than CAP above the
    # minimum running depth of both segments (a closing bracket further above its segment's has no room in its list,
    # an opening one none in its own)
    low_a = np.array(low, dtype=np.int64)
    g = partner[p:]
    t = np.flatnonzero((g != NONE) & (g >= p) & (g - p > np.arange(n)))  # opening brackets with a partner in the shard
    u = g[t] - p
    q, sc, c = seg[t], seg[u], e.dep[t].astype(np.int64)
    cross = q != sc
    cut_close = cross & (c - low_a[sc] >= CAP)
    cut_open = cross & ~cut_close & (c - low_a[q] >= CAP)
    keep = ~(cut_close | cut_open)
    e.match = np.full(n, NONE, dtype=np.int64)
    e.match[t[keep]], e.match[u[keep]] = pos[u[keep]], pos[t[keep]]
    e.crossing, e.cut = int(cross.sum()), int((~keep).sum())
    # bit 31: a segment behind the first with more closing brackets than its list holds, or an opening bracket the
    # stitch found outside its segment's list
    e.clipped = any(start[s] - low[s] > CAP for s in range(1, len(bases))) or bool(cut_open.any())
    # the header's promise, independently of the model above: every container less than CAP levels above the shard's
    # minimum running depth is stitched
    assert keep[c - min(low) < CAP].all(), case.name
    e.pos, e.seg = pos, seg
    return e


# ---- CPU: the definition the GPU test uses, against a plain statement ----------------------------------------------
def _stack_match(types):
    out, stack = [NONE] * len(types), []
    for i, c in enumerate(types):
        if c in OPEN:
            stack.append(i)
        elif c in CLOSE and stack:
            o = stack.pop()
            out[i], out[o] = o, i
    return out


def _plain_depths(types, d=0):
    out = []
    for c in types:
        if c in CLOSE:
            d -= 1
        out.append(d)
        if c in OPEN:
            d += 1
    return out


def _all_cases():
    return random_cases() + placement_cases() + prev_cases() + clip_cases()


def test_case_generator_against_a_plain_stack():
    """The cases' token streams: the partners and depths helpers.oracle_* give (what the GPU test compares with) are
    those of a plain Python stack; and the cases reach what they are there for."""
    deepest, empties, crossing, prevs = 0, 0, 0, set()
    for case in _all_cases():
        idx = _index(case.data)
        typ, dep, _ = helpers.oracle_tokens(case.data, idx)
        types = bytes(typ)
        assert helpers.oracle_match(typ).astype(np.int64).tolist() == _stack_match(types), case.name
        assert dep.tolist() == _plain_depths(types), case.name
        e = _expected(case, idx)
        assert len(e.segs) <= 32 and sum(s[3] for s in e.segs) == len(types) - e.prefix_n, case.name
        # the shard's own stack: a partner inside the shard is the whole stream's partner
        own = _stack_match(types[e.prefix_n:])
        want = [NONE if m == NONE else int(e.pos[m]) for m in own]
        if not e.clipped:
            assert e.match.tolist() == want, case.name
        deepest = max(deepest, max(d - e.low[0] for d in e.dep.tolist()) if len(types) else 0)
        empties += sum(1 for s in e.segs[1:-1] if s[3] == 0)
        crossing += e.crossing
        if e.prefix_n:
            prevs.add(e.prefix_final)
    assert deepest > CAP and empties >= 2 and crossing > 100000 and prevs == {37, -5, 9008}


def test_case_generator_reaches_its_edges():
    """The placement case: a border in front of and behind a bracket, partners one and several segments back,
    across a segment that closes a level and opens it again, in front of the shard, never closed; segments without
    a token."""
    case = placement_cases()[0]
    e = _expected(case)
    bracket = np.isin(e.typ, list(OPEN + CLOSE))
    first_of = {s[2] for s in e.segs if s[3]}
    last_of = {s[2] + s[3] - 1 for s in e.segs if s[3]}
    assert any(bracket[t] for t in first_of) and any(bracket[t] for t in last_of)
    back = [int(e.seg[t]) - int(e.seg[np.searchsorted(e.pos, e.match[t])]) for t in range(e.typ.size)
            if e.typ[t] in CLOSE and e.match[t] != NONE]
    assert 0 in back and 1 in back and max(back) >= 3
    assert ((e.match == NONE) & bracket).sum() >= 5  # in front of the shard / never closed
    # segments without a token in the middle of a shard, their (unread) index slices off the 16-byte grid
    empty = [sg for c in placement_cases() for sg in _expected(c).segs[1:-1] if sg[3] == 0]
    assert empty and all(sg[2] % 4 for sg in empty)


# ---- GPU --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.close()


def _call(dev, shard, segs, idx_rel, match=True, prev=None, fill=0x5A):
    """msj_stage2_prep_segments on output arrays filled with a pattern; -> (rc, offsets, type, depth, match, results)."""
    import torch
    from mojo_simdjson_amd import _lib

    dv = dev.device
    L = dev.lib
    L.msj_stage2_prep_segments.restype = ctypes.c_int32
    nseg = len(segs)
    table = (_lib.MsjSegment * nseg)()
    for k, (bb, bl, ib, cnt) in enumerate(segs):
        table[k].byte_base, table[k].byte_len, table[k].index_begin, table[k].count = bb, bl, ib, cnt
    total = max(sum(_round8(s[3]) for s in segs), 8)
    d_buf = torch.from_numpy(np.frombuffer(shard + b" " * 64, dtype=np.uint8).copy()).to(dv)
    d_idx = torch.from_numpy(np.concatenate([idx_rel, np.zeros(8, np.int64)]).astype(np.uint32).view(np.int32)).to(dv)
    d_type = torch.full((total,), fill, dtype=torch.uint8, device=dv)
    d_depth = torch.full((total,), fill * 0x01010101, dtype=torch.int32, device=dv)
    d_match = torch.full((total,), fill * 0x01010101, dtype=torch.int32, device=dv) if match else None
    d_end = torch.full((total,), fill * 0x01010101, dtype=torch.int32, device=dv)
    d_flags = torch.full((total,), fill, dtype=torch.uint8, device=dv)
    d_res = torch.full((24 * nseg,), fill, dtype=torch.uint8, device=dv)
    d_prev = None
    if prev is not None:
        r = _lib.MsjTokensResult(*prev)
        d_prev = torch.frombuffer(bytearray(bytes(r)), dtype=torch.uint8).to(dv)
    offs = (ctypes.c_uint64 * nseg)()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    rc = L.msj_stage2_prep_segments(dev.ctx, p(d_buf), ctypes.byref(table), nseg, p(d_idx), p(d_type), p(d_depth), p(d_match),
                                    p(d_end), p(d_flags), p(d_res), p(d_prev), offs, dev._stream())
    torch.cuda.synchronize(dv)
    raw = d_res.cpu().numpy().tobytes()
    results = [_lib.MsjTokensResult.from_buffer_copy(raw[24 * k:24 * k + 24]) for k in range(nseg)]
    out = dict(type=d_type.cpu().numpy(), depth=d_depth.cpu().numpy(), end=d_end.cpu().numpy(), flags=d_flags.cpu().numpy(),
               match=d_match.cpu().numpy().view(np.uint32).astype(np.int64) if match else None, raw_results=raw)
    return rc, [int(o) for o in offs], out, results


def _gather(arr, e):
    return np.concatenate([arr[o:o + s[3]] for o, s in zip(e.offs, e.segs)]) if e.segs else arr[:0]


def _check(dev, case, e=None):
    e = _expected(case) if e is None else e
    prev = e.prefix_result if case.prefix else None
    rc, offs, out, results = _call(dev, case.data[case.prefix:], e.segs, e.idx_rel, prev=prev)
    where = case.name
    assert rc == 0 and offs == e.offs, (where, rc)
    assert np.array_equal(_gather(out["type"], e), e.typ), where
    got_d = _gather(out["depth"], e)
    if not np.array_equal(got_d, e.dep):
        bad = int(np.argmax(got_d != e.dep))
        raise AssertionError(f"{where}: depth of token {bad} = {got_d[bad]} != {e.dep[bad]}")
    got_m = _gather(out["match"], e)
    if not np.array_equal(got_m, e.match):
        bad = np.flatnonzero(got_m != e.match)
        t = int(bad[0])
        raise AssertionError(f"{where}: {bad.size} partners differ; token {t} (segment {int(e.seg[t])}, type {chr(e.typ[t])}, "
                             f"depth {int(e.dep[t])}): {got_m[t]:#x} != {e.match[t]:#x}")
    for s, (r, w) in enumerate(zip(results, e.results)):
        opens = r.reserved & 0x7FFFFFFF if s == len(results) - 1 else r.reserved
        assert (r.n, r.final_depth, r.min_depth, r.max_depth, opens) == w, (where, s, (r.n, r.final_depth, r.min_depth, r.max_depth, opens), w)
    assert results[-1].reserved >> 31 == int(e.clipped), where
    return e, results


@pytest.mark.gpu
def test_random_depth_profiles(dev):
    """Seeded ramps to ~20 000 levels, sawtooths, plateaus, descents below the start, over 2 .. 32 segments of 4 KiB,
    8 KiB, 64 KiB and 1 MiB: every partner, type, depth and result."""
    crossing = 0
    for case in random_cases():
        e, _ = _check(dev, case)
        assert not e.clipped and e.cut == 0, case.name
        crossing += e.crossing
    assert crossing > 1000


@pytest.mark.gpu
def test_partner_placements_and_token_edges(dev):
    """Partners in the same segment, one back, several back over segments that never reach the level or close it and
    open it again, in front of the shard, never closed; borders right before and behind a bracket, inside strings
    full of brackets; segments without a token; shards of closing brackets only and of opening brackets only."""
    for case in placement_cases():
        e, _ = _check(dev, case)
        assert not e.clipped, case.name
    assert any(s[3] == 0 for s in _expected(placement_cases()[2]).segs[1:-1])


@pytest.mark.gpu
def test_shard_that_starts_inside_its_stream(dev):
    """d_prev set: the shard starts at depth 37 of its stream, and at -5, and goes below that.  Depths, results and
    partners are those of the same tokens inside the longer stream, except partners in front of the shard."""
    for case in prev_cases():
        e, results = _check(dev, case)
        assert min(e.low) < e.prefix_final, case.name  # it goes below its start
        assert results[-1].min_depth == e.results[-1][2]


@pytest.mark.gpu
def test_clip_keeps_the_levels_nearest_the_minimum(dev):
    """More than MSJ_RESID_CAP levels at a border: bit 31 of the last result is set, and exactly the containers more than
    CAP levels above the minimum of one of their two segments keep 0xFFFFFFFF -- the root and the levels near it are
    stitched (include/msj_stage1.h)."""
    for case in clip_cases():
        e, results = _check(dev, case)
        assert e.clipped and results[-1].reserved >> 31 == 1, case.name
    # the issue's own example: depths 0 .. 65 535 stitched, 65 536 .. 69 631 cut, the rest paired inside segment 1
    e = _expected(clip_cases()[0])
    opens = np.flatnonzero(e.typ == ord("["))
    assert (e.match[opens[:CAP]] != NONE).all() and (e.match[opens[CAP:69632]] == NONE).all() and (e.match[opens[69632:]] != NONE).all()


@pytest.mark.gpu
def test_clip_through_the_shard_call(dev):
    """The 70 000-deep case with the segment table msj_stage1_shard_device cuts (69 632-byte segments forced by the test
    hook) and the shard's own index array."""
    import torch

    case = clip_cases()[0]
    data = case.data
    L = dev.lib
    L.msj_debug_set_segment_bytes.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    assert L.msj_debug_set_segment_bytes(dev.ctx, 69632) == 0
    try:
        d_buf = torch.from_numpy(np.frombuffer(data + b" " * 64, dtype=np.uint8).copy()).to(dev.device)
        d_idx = torch.empty(len(data) + 64, dtype=torch.int32, device=dev.device)
        d_seg = torch.zeros(32 * 8, dtype=torch.uint8, device=dev.device)
        cin, cout = dev.make_carry(0, 0, 0), dev.new_carry()
        _, nseg = dev.shard(d_buf, len(data), d_idx, cin, cout, segments=d_seg, is_final=True, trailer_len=len(data))
        assert nseg == 3 and dev.fetch(cout).code == 0
        segs = [tuple(int(x) for x in row) for row in np.frombuffer(d_seg.cpu().numpy().tobytes(), dtype=np.uint64).reshape(8, 4)[:nseg]]
        e = _expected(case)
        assert [(s[0], s[2], s[3]) for s in segs] == [(s[0], s[2], s[3]) for s in e.segs]
        offs, t, d, m, _, _, results = dev.stage2_prep_segments(d_buf, segs, d_idx, match=True)
        assert offs == e.offs
        got_m = _gather(m.cpu().numpy().view(np.uint32).astype(np.int64), e)
        assert np.array_equal(got_m, e.match)
        assert np.array_equal(_gather(d.cpu().numpy(), e), e.dep)
        assert results[-1].reserved >> 31 == 1
    finally:
        assert L.msj_debug_set_segment_bytes(dev.ctx, 0xFFFF0000) == 0


@pytest.mark.gpu
def test_segment_limits(dev):
    """33 segments with d_match: MSJ_CAPACITY, nothing launched (every output array keeps its pattern); the same table
    without d_match succeeds; one segment with d_match gives the partners of msj_stage2_prep_chain_device."""
    import torch

    data = random_profile(3, "saw", 33 * 4096)
    case = Case("33 segments", data, [len(data) * k // 33 // 16 * 16 for k in range(1, 33)])
    e = _expected(case)
    assert len(e.segs) == 33
    rc, _, out, _ = _call(dev, data, e.segs, e.idx_rel, match=True)
    assert rc == MSJ_CAPACITY
    assert (out["type"] == 0x5A).all() and (out["flags"] == 0x5A).all()
    assert (out["depth"] == 0x5A5A5A5A).all() and (out["end"] == 0x5A5A5A5A).all() and (out["match"] == 0x5A5A5A5A).all()
    assert set(out["raw_results"]) == {0x5A}
    rc, offs, out, results = _call(dev, data, e.segs, e.idx_rel, match=False)
    assert rc == 0 and offs == e.offs
    assert np.array_equal(_gather(out["depth"], e), e.dep) and np.array_equal(_gather(out["type"], e), e.typ)
    assert [(r.n, r.final_depth, r.min_depth, r.max_depth) for r in results] == [w[:4] for w in e.results]

    one = random_profile(4, "saw", 50000)
    for case in (Case("one segment", one, []), Case("one segment, d_prev", b"[" * 48 + one, [], prefix=48)):
        e = _expected(case)
        e1, _ = _check(dev, case)
        shard = case.data[case.prefix:]
        d_buf = torch.from_numpy(np.frombuffer(shard + b" " * 64, dtype=np.uint8).copy()).to(dev.device)
        d_idx = torch.from_numpy(np.concatenate([e.idx_rel, np.zeros(8, np.int64)]).astype(np.uint32).view(np.int32)).to(dev.device)
        d_prev = None
        if case.prefix:
            from mojo_simdjson_amd import _lib

            d_prev = torch.frombuffer(bytearray(bytes(_lib.MsjTokensResult(*e.prefix_result))), dtype=torch.uint8).to(dev.device)
        _, _, _, m, _, _ = dev.stage2_prep(d_buf, len(shard), d_idx, e.idx_rel.size, match=True, d_prev=d_prev)
        assert np.array_equal(m.cpu().numpy().view(np.uint32).astype(np.int64), e1.match), case.name
