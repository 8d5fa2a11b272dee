"""msj_match_strings_device in stream order (the manner of tests/test_dictionary_order_stream_order.py; the delay and its
bounds are tests/test_stream_order.py's): on a side stream, behind a column that arrives late, with sync=False and every
output a tensor of the caller's.

The decoy B -- A's row lengths, other bytes -- lies in the column tensors and has been through the calls: one call of
single-piece patterns and one of patterns of up to four pieces.  Every tensor and the workspace hold B's consistent state.
Then, on a side stream: a delay, device-to-device copies of A's bytes and validity over them, the outputs back to their fill,
and the calls.  A launch or a memset that dropped its stream argument runs ahead of the copies and reads the decoy; what it
writes is then overwritten with the fill or differs from A's expected arrays, which come from the host twin alone.  With
nullptr for `stream` at msj_launch_match_strings (tried once on a copy of the tree) the test fails at the first call's
`fields0`, all 256 000 bytes of which still hold their fill: the kernels ran on the null stream ahead of the side stream's
copies and the reset.

The second set-up runs two contexts on two streams in turns, A on one and B on the other, with nothing waited for.
"""
import random

import numpy as np
import pytest

from tests import test_match_strings_math as tmm
from tests import test_stream_order as tso
from tests import test_tape_documents as ttd

ROWS = 4000
SPECS = ([b"ab", ([b"ba"], tmm.AT_END), ([b"AB"], tmm.NOCASE | tmm.AT_START), b"a"],
         [([b"a", b"b", b"a"], 0), ([b"ab", b"ab", b"a", b"b"], tmm.AT_END), b"bab", ([b"B", b"A"], tmm.NOCASE)])
FLAG_NAMES = ((tmm.AT_START, "at_start"), (tmm.AT_END, "at_end"), (tmm.NOCASE, "nocase"))


def wrapper_specs(specs):
    return [(tmm.norm(s)[0], {name for bit, name in FLAG_NAMES if tmm.norm(s)[1] & bit}) for s in specs]


class Expected:
    """The calls over one column on the host"""

    def __init__(self, decoy):
        tw = tmm.load_twin()
        lengths = random.Random(5)   # A's and the decoy's rows have the same lengths: the offsets agree, a call's sizes too
        rng = random.Random(77 if decoy else 7)
        rows = []
        for _ in range(ROWS):
            ln = lengths.choice((0, 2, 5, 9, 33, 120))
            rows.append(tmm.word(rng, ln, tmm.ALPHABET[1:4]) if rng.random() > 0.05 else ("null", tmm.word(rng, ln, tmm.ALPHABET[1:4])))
        self.col = tmm.Column(rows)
        self.out = []
        for specs in SPECS:
            rc, res, sel, rec = tmm.run_twin(tw, self.col, specs)
            assert rc == 0 and res.code == 0 and res.n_matched > ROWS // 4
            self.out.append((res, sel, rec))

    def arrays(self):
        """{name: the expected bytes}, in the order of the calls"""
        raw = lambda s: np.frombuffer(bytes(s), dtype=np.uint8)
        out = {}
        for j, (res, sel, rec) in enumerate(self.out):
            out.update({f"fields{j}": np.frombuffer(rec.tobytes(), dtype=np.uint8), f"res{j}": raw(res), f"sel{j}": raw(sel)})
        return out


def test_expected_on_cpu():
    """A's and the decoy's expected arrays have the same sizes and differ in every array a call writes: a call that read the
    decoy shows"""
    a, b = Expected(False), Expected(True)
    assert np.array_equal(a.col.offsets, b.col.offsets) and a.col.data != b.col.data
    for name, want in a.arrays().items():
        other = b.arrays()[name]
        assert want.size == other.size and not np.array_equal(want, other), name


class Tensors:
    """The column and the caller's output tensors of the calls on one device"""

    def __init__(self, dev, x, start):
        self.dev, self.x = dev, x
        self.d_offsets = ttd.to_device(dev, start.col.offsets.view(np.int64))
        self.d_valid, self.d_bytes = ttd.to_device(dev, start.col.valid), ttd.to_device(dev, np.frombuffer(start.col.data, dtype=np.uint8).copy())
        self.patterns = [dev.compile_patterns(wrapper_specs(s)) for s in SPECS]
        self.out = {name: ttd.to_device(dev, np.full(w.size, 0xA5, dtype=np.uint8)) for name, w in x.arrays().items()}
        self.pristine = {name: t.clone() for name, t in self.out.items()}

    def copy_in(self, other):
        self.d_valid.copy_(other.d_valid, non_blocking=True)
        self.d_bytes.copy_(other.d_bytes, non_blocking=True)

    def reset(self):
        for name, t in self.out.items():
            t.copy_(self.pristine[name], non_blocking=True)

    def call(self, j):
        import torch

        n = len(SPECS[j])
        self.dev.match_strings(self.patterns[j], self.d_offsets, self.d_valid, self.d_bytes, rows=ROWS,
                               d_fields=self.out[f"fields{j}"].view(torch.int64).view(n, ROWS, 2), d_result=self.out[f"res{j}"],
                               d_select=self.out[f"sel{j}"], sync=False)

    def check(self, want, where):
        for name, w in want.items():
            got = self.out[name].cpu().numpy()
            bad = np.nonzero(got != w)[0]
            assert bad.size == 0, (where, name, int(bad[0]) // 16, got[bad[:4]].tolist(), w[bad[:4]].tolist(), int(bad.size))


N_CALLS = len(SPECS)


@pytest.mark.gpu
def test_match_behind_a_late_column(dev):
    import time

    import torch

    a, b = Expected(False), Expected(True)
    t, source = Tensors(dev, a, b), Tensors(dev, a, a)

    def enqueue():
        t.reset()
        for j in range(N_CALLS):
            t.call(j)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enqueue()   # the decoy through the calls: the workspace has its size and holds its state
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    t.check(b.arrays(), "the decoy")
    s = torch.cuda.Stream(dev.device)
    need_ms = max(tso.MIN_DELAY_MS, tso.JITTER * t_enq * 1e3)
    start, ready = tso.delayed(s, need_ms), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        t.copy_in(source)
        ready.record()
        enqueue()
    pending = not ready.query()
    s.synchronize()
    delay_ms = start.elapsed_time(ready)
    numbers = f"the enqueue took {t_enq * 1e3:.2f} ms on the host, the delay {delay_ms:.1f} ms of the {need_ms:.1f} ms it has to last"
    print(numbers)
    assert pending, "inconclusive: the column was there when the enqueue returned -- a host wait in the call, or the delay too short: " + numbers
    assert delay_ms >= need_ms, numbers
    t.check(a.arrays(), "behind a late column")


@pytest.mark.gpu
def test_two_contexts_two_streams():
    """Two contexts on two side streams, A on one and the decoy B on the other, the calls enqueued in turns with nothing waited
    for: device state that the process holds once would be shared by the two"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    devs = [Stage1Device(0), Stage1Device(0)]
    try:
        windows = [Expected(False), Expected(True)]
        sets = [Tensors(d, x, x) for d, x in zip(devs, windows)]
        for t in sets:   # every workspace has its size
            t.call(0)
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(d.device) for d in devs]
        for s, t in zip(streams, sets):
            with torch.cuda.stream(s):
                t.reset()
        for _ in range(3):
            for j in range(N_CALLS):
                for s, t in zip(streams, sets):
                    with torch.cuda.stream(s):
                        t.call(j)
        for s in streams:
            s.synchronize()
        for t, x in zip(sets, windows):
            t.check(x.arrays(), "two contexts")
    finally:
        for d in devs:
            d.close()


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.close()
