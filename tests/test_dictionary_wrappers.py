"""Stage1Device.dictionary (mojo_simdjson_amd/device.py) as a wrapper, the way tests/test_column_wrappers.py pins its five
siblings: over the window of that file -- the strings of /s, the keys of the map /m, and the path no document has -- these
ways of calling give the same codes, dictionary (cut at the counts the call reports) and the same result struct:
    1. everything defaulted -- the layout-only first call plus the real call
    2. the caller's d_codes and dictionary buffers, no capacity named
    3. capacities named, no buffers
    4. sync=False: the device tensor that holds the result, its bytes those of the synchronous result
and the layout-only form alone returns None for the dictionary and the same codes and counts.  d_n_rows on the device (the
n_rows word of the string column's own result) gives what `rows` gives.  The first way is held against dict.setdefault.
"""
import numpy as np
import pytest

from tests import test_column_wrappers as tcw
from tests import test_dictionary_math as tdc

pytestmark = pytest.mark.gpu


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
def win(dev):
    return tcw.Win(dev)


def held(dev, d_offsets, d_bytes, d_valid, rows, d_string_result):
    """The ways of calling against each other -> (result, codes[R], the distinct values)"""
    import torch

    call = lambda **kw: dev.dictionary(d_offsets, d_bytes, d_valid, rows=rows, **kw)
    first = call()
    res = first[0]
    R, n, total = int(res.n_rows), int(res.n_distinct), int(res.dict_bytes)
    assert R == rows and res.code == 0

    def view(got):
        assert len(got) == 5
        return got[1].cpu().numpy()[:R], got[2].cpu().numpy()[:n + 1], got[3].cpu().numpy()[:n], got[4].cpu().numpy()[:total]

    def same(got, where):
        assert all(np.array_equal(x, y) for x, y in zip(view(got), view(first))), where

    plain = lambda r: bytes(r)[:40]   # (everything but max_probe, which is no function of the input alone)
    # 1: sized from the layout-only first call, never an empty tensor
    assert first[1].dtype == torch.int32 and first[1].numel() == max(rows, 1) and first[2].numel() == n + 1
    assert first[3].numel() == max(n, 1) and first[4].numel() == max(total, 1)
    # the layout-only form alone
    layout = call(values=False)
    assert all(t is None for t in layout[2:]) and plain(layout[0]) == plain(res) and np.array_equal(layout[1].cpu().numpy()[:R], view(first)[0])
    # 2: the caller's buffers, no capacity named
    mine = dict(d_codes=torch.full((max(rows, 1),), 0x77, dtype=torch.int32, device=dev.device),
                d_dict_offsets=torch.full((n + 1,), 0x77, dtype=torch.int64, device=dev.device),
                d_dict_first=torch.full((max(n, 1),), 0x77, dtype=torch.int32, device=dev.device),
                d_dict_bytes=torch.full((max(total, 1),), 0x77, dtype=torch.uint8, device=dev.device))
    second = call(**mine)
    assert all(second[1 + j] is mine[name] for j, name in enumerate(("d_codes", "d_dict_offsets", "d_dict_first", "d_dict_bytes")))
    assert plain(second[0]) == plain(res)
    same(second, 2)
    # 3: capacities named, no buffers
    third = call(dict_capacity=n, dict_bytes_capacity=total)
    assert plain(third[0]) == plain(res) and third[3].numel() == max(n, 1) and third[4].numel() == max(total, 1)
    same(third, 3)
    # 4: nothing waited for
    fourth = call(sync=False)
    assert isinstance(fourth[0], torch.Tensor) and fourth[0].is_cuda and fourth[0].cpu().numpy().tobytes()[:40] == plain(res)
    same(fourth, 4)
    # the rows on the device: the n_rows word of the column call's own result, no capacity named
    fifth = dev.dictionary(d_offsets, d_bytes, d_valid, d_n_rows=d_string_result[8:16].view(torch.int64))
    assert plain(fifth[0]) == plain(res)
    same(fifth, 5)
    with pytest.raises(ValueError):
        call(d_dict_offsets=mine["d_dict_offsets"])
    codes, off, _, data = view(first)
    return res, codes.tolist(), [data[off[c]:off[c + 1]].tobytes() for c in range(n)]


def check(dev, win, d_fields, p, d_sel, rows, want):
    d_res, d_off, d_valid, d_bytes = dev.string_column(win.a.d_buf, win.a.length, d_fields, p, d_sel, sync=False)
    res, codes, values = held(dev, d_off, d_bytes, d_valid, rows, d_res)
    want_codes, distinct, _ = tdc.definition(want)
    assert (codes, values) == (want_codes, distinct) and (res.n_values, res.n_distinct) == (sum(v is not None for v in want), len(distinct))
    return values


def test_strings_of_a_path(dev, win):
    want = [v.encode() if isinstance(v, str) else None for v in (tcw.ref.lookup(tcw.ref.decode(text), "/s")[1] for text in tcw.LINES)]
    assert check(dev, win, win.d_fields, 0, win.d_sel, win.D, want) == [b"red", b"a\nb"]
    assert check(dev, win, win.d_fields, tcw.MISSING, win.d_sel, win.D, [None] * win.D) == []


def test_keys_of_a_map(dev, win):
    import json

    _, _, _, d_keys, _, d_ksel, _ = dev.object_entries(*win.tokens, win.d_fields[tcw.POINTERS.index("/m")], win.d_sel, sync=False, **win.numbers)
    pairs = [k for text in tcw.LINES for k, _ in (json.loads(text, object_pairs_hook=list)[-1][1] if b'"m":{' in text else [])]
    assert pairs == ["color", "size", "k", "k2"]
    assert check(dev, win, d_keys.unsqueeze(0), 0, d_ksel, len(pairs), [k.encode() for k in pairs]) == [k.encode() for k in pairs]
