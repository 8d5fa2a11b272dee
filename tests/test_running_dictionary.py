"""RunningDictionary (mojo_simdjson_amd/document_stream.py) without a GPU: its bookkeeping -- the entries held, the growth on
a clipped call and the repeat with the same number of prior entries, the views it hands out, the -1 in ``first`` for values
of earlier windows, the frozen form, the error for any other code -- over a stand-in for Stage1Device whose
``dictionary_extend`` is the host twin of the call (tests/dictionary_extend_math_host.cpp) on CPU tensors.  The real chain
on the device is tests/test_dictionary_extend.py's end-to-end test."""
import ctypes

import pytest

from mojo_simdjson_amd import _lib
from tests import test_dictionary_extend_math as txm


class TwinDevice:
    """``Stage1Device.dictionary_extend`` as RunningDictionary calls it, computed by the twin"""

    device = "cpu"

    def __init__(self):
        self.twin, self.calls = txm.load_twin(), []

    def dictionary_extend(self, d_offsets, d_bytes, d_valid, d_dict_offsets, d_dict_first, d_dict_bytes, n_prior=0, rows=None, frozen=False):
        import torch

        d_codes = torch.zeros(max(rows, 1), dtype=torch.int32)
        res = _lib.MsjDictionaryExtendResult()
        self.calls.append((n_prior, d_dict_first.numel(), d_dict_bytes.numel()))
        self.twin.dxm_dictionary_extend(d_offsets.data_ptr(), d_valid.data_ptr(), rows, None, d_bytes.data_ptr(), d_bytes.numel(), n_prior, None,
                                        d_codes.data_ptr(), d_dict_offsets.data_ptr(), d_dict_first.data_ptr(), d_dict_first.numel(),
                                        d_dict_bytes.data_ptr(), d_dict_bytes.numel(), txm.FROZEN if frozen else 0, 0, ctypes.byref(res))
        return res, d_codes, d_dict_offsets, d_dict_first, d_dict_bytes


def column(values):
    """Python strings (None: a row without one) -> (offsets, bytes, valid) as the column calls return them"""
    import torch

    col = txm.column_of([v.encode() if v is not None else None for v in values])
    return (torch.from_numpy(col.offsets.view("int64")), torch.from_numpy(col.data), torch.from_numpy(col.valid).view(torch.bool))


def test_windows_grow_one_dictionary():
    torch = pytest.importorskip("torch")
    from mojo_simdjson_amd.document_stream import DocumentStreamError, RunningDictionary

    dev = TwinDevice()
    rd = RunningDictionary(dev, dict_capacity=2, bytes_capacity=8)
    assert (rd.n_distinct, rd.dict_capacity, rd.bytes_capacity, rd.values()) == (0, 2, 8, [])
    first = rd.encode(column(["error", None, "ok", "error"]))
    assert first.codes.tolist() == [0, -1, 1, 0] and first.first.tolist() == [0, 2] and rd.values() == ["error", "ok"] == first.values()
    assert dev.calls == [(0, 2, 8)]   # it fitted: one call
    second = rd.encode(column(["ok", "warning", "", "debug", "warning", "error"]))
    assert second.codes.tolist() == [1, 2, 3, 4, 2, 0] and second.first.tolist() == [-1, -1, 1, 2, 3]
    assert rd.values() == ["error", "ok", "warning", "", "debug"] == second.values() and rd.n_distinct == second.n_distinct == 5
    assert second.counts().tolist() == [1, 1, 2, 1, 1]
    # clipped once, grown to at least the double and at least what the result named, repeated with the same prior entries
    assert dev.calls[1:] == [(2, 2, 8), (2, 5, 19)] and (rd.dict_capacity, rd.bytes_capacity) == (5, 19)
    assert first.values() == ["error", "ok"] and first.offsets.tolist() == [0, 5, 7]   # the earlier column keeps its tensors
    third = rd.encode(column(["trace", "ok"]), frozen=True)
    assert third.codes.tolist() == [-2, 1] and third.first.tolist() == [-1] * 5 and rd.n_distinct == 5 and len(dev.calls) == 4
    empty = rd.encode(column([]))
    assert empty.codes.tolist() == [] and empty.n_distinct == 5
    fourth = rd.encode(column(["x" * 40]))
    assert fourth.codes.tolist() == [5] and (rd.dict_capacity, rd.bytes_capacity) == (10, 59) and rd.values()[-1] == "x" * 40
    # any other code: the arrays' own offsets say more bytes than there is room for
    rd.offsets[rd.n_distinct] = rd.bytes_capacity + 1
    with pytest.raises(DocumentStreamError):
        rd.encode(column(["ok"]))
    assert torch.equal(rd.offsets[:3], first.offsets)
