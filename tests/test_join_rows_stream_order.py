"""msj_join_rows_device in stream order (the manner of tests/test_sort_rows_stream_order.py; the delay and its bounds are
tests/test_stream_order.py's): on a side stream, behind inputs that arrive late, with sync=False, the rooms given and every
output a tensor of the caller's.

The decoy B -- A's sizes, other keys -- lies in both key columns and has been through the three joins (INNER with the
offsets, LEFT, SEMI without a right vector): every tensor and the workspace hold B's consistent state.  Then, on a side
stream: a delay, device-to-device copies of A's two key columns over them, the outputs back to their fill, and the joins.  A
launch or a memset that dropped its stream argument runs ahead of the copies and reads the decoy; what it writes is then
overwritten with the fill or differs from A's expected arrays, which come from the host twin (tests/join_rows_math_host.cpp)
alone.  With nullptr for `stream` at msj_launch_join_rows (tried once on a copy of the tree) the test fails at the first
join's pairs: the kernels ran on the null stream ahead of the side stream's copies.

The second set-up runs two contexts on two streams in turns, A on one and B on the other, with nothing waited for.
"""
import numpy as np
import pytest

from tests import test_join_rows_math as tjm
from tests import test_stream_order as tso
from tests import test_tape_documents as ttd

LEFT_ROWS, RIGHT_ROWS, KEYS, ROOM = 6000, 5000, 900, 60000
CALLS = (("inner", True, True), ("left", True, False), ("semi", False, False))     # how, with d_right_rows, with d_offsets
KIND = {"inner": tjm.INNER, "left": tjm.LEFT, "semi": tjm.SEMI}


def make_keys(seed):
    rng = np.random.default_rng(seed)
    draw = lambda n: np.where(rng.random(n) < 0.1, -1, rng.integers(0, KEYS, n)).astype(np.int32)
    return draw(LEFT_ROWS), draw(RIGHT_ROWS)


class Expected:
    """The three joins over one pair of key columns on the host"""

    def __init__(self, decoy):
        tw = tjm.load_twin()
        self.lk, self.rk = make_keys(77 if decoy else 7)
        self.joined = [tjm.twin_join(tw, self.lk, self.rk, KEYS, KIND[how], pairs_capacity=ROOM, want_right=right, want_offsets=offsets)
                       for how, right, offsets in CALLS]
        assert all(j.rc == 0 and j.res.code == 0 and j.res.n_pairs >= 1000 for j in self.joined)

    def arrays(self):
        """{name: the expected bytes}"""
        out = {}
        for j, (x, (_, right, offsets)) in enumerate(zip(self.joined, CALLS)):
            out.update({f"left{j}": x.left.view(np.uint8), f"res{j}": np.frombuffer(bytes(x.res), dtype=np.uint8),
                        f"lsel{j}": np.frombuffer(bytes(x.lsel), dtype=np.uint8), f"rsel{j}": np.frombuffer(bytes(x.rsel), dtype=np.uint8)})
            if right:
                out[f"right{j}"] = x.right.view(np.uint8)
            if offsets:
                out[f"offsets{j}"] = x.offsets.view(np.uint8)
        return out


def test_expected_on_cpu():
    """A's and the decoy's expected arrays have the same sizes and differ in the pairs of every join: a join that read the decoy
    shows"""
    a, b = Expected(False), Expected(True)
    for name, want in a.arrays().items():
        other = b.arrays()[name]
        assert want.size == other.size and (not name.startswith(("left", "right", "offsets")) or not np.array_equal(want, other)), name


class Tensors:
    """The inputs and the caller's output tensors of the three joins on one device"""

    def __init__(self, dev, x, start):
        self.dev, self.x = dev, x
        self.d_lk, self.d_rk = ttd.to_device(dev, start.lk), ttd.to_device(dev, start.rk)
        self.out = {name: ttd.to_device(dev, np.full(w.size, tjm.FILL, dtype=np.uint8)) for name, w in x.arrays().items()}
        self.pristine = {name: t.clone() for name, t in self.out.items()}

    def copy_in(self, other):
        self.d_lk.copy_(other.d_lk, non_blocking=True)
        self.d_rk.copy_(other.d_rk, non_blocking=True)

    def reset(self):
        for name, t in self.out.items():
            t.copy_(self.pristine[name], non_blocking=True)

    def call(self, j):
        import torch

        how, right, offsets = CALLS[j]
        self.dev.join_rows(self.d_lk, self.d_rk, n_keys=KEYS, how=how, pairs_capacity=ROOM, d_left_rows=self.out[f"left{j}"].view(torch.int32),
                           d_right_rows=self.out[f"right{j}"].view(torch.int32) if right else None, right=right,
                           d_offsets=self.out[f"offsets{j}"].view(torch.int64) if offsets else None, d_result=self.out[f"res{j}"],
                           d_left_select=self.out[f"lsel{j}"], d_right_select=self.out[f"rsel{j}"], sync=False)

    def check(self, want, where):
        for name, w in want.items():
            got = self.out[name].cpu().numpy()
            bad = np.nonzero(got != w)[0]
            assert bad.size == 0, (where, name, int(bad[0]) // 4, got[bad[:4]].tolist(), w[bad[:4]].tolist(), int(bad.size))


@pytest.mark.gpu
def test_join_rows_behind_late_inputs(dev):
    import time

    import torch

    a, b = Expected(False), Expected(True)
    t, source = Tensors(dev, a, b), Tensors(dev, a, a)

    def enqueue():
        t.reset()
        for j in range(len(CALLS)):
            t.call(j)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enqueue()   # the decoy through the joins: the workspace has its size and holds its state
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
    assert pending, "inconclusive: the inputs were there when the enqueue returned -- a host wait in the call, or the delay too short: " + numbers
    assert delay_ms >= need_ms, numbers
    t.check(a.arrays(), "behind late inputs")


@pytest.mark.gpu
def test_two_contexts_two_streams():
    """Two contexts on two side streams, A on one and the decoy B on the other, the joins enqueued in turns with nothing waited
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
            for j in range(len(CALLS)):
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
