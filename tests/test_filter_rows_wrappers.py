"""The predicate specs of Stage1Device.compile_predicates and of the where methods, without a device: what a tuple becomes
as a msj_predicate (mojo_simdjson_amd.device.predicate_struct), what is rejected, and how the document-stream layer names
columns (mojo_simdjson_amd.document_stream._column_specs).  The host twin's compile step takes every struct made here."""
import ctypes
import struct

import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.device import predicate_struct
from mojo_simdjson_amd.document_stream import _column_specs
from tests import test_filter_rows_math as tfm


def fields(p):
    return (p.column, p.op, p.flags, p.operand_len, p.operand_bits)


def test_specs_become_predicates():
    alive = []
    made = lambda spec: predicate_struct(spec, alive)
    assert fields(made((0, "found"))) == (0, _lib.PRED_FOUND, 0, 0, 0)
    assert fields(made(("not", (3, "found")))) == (3, _lib.PRED_FOUND, _lib.PRED_NOT, 0, 0)
    assert fields(made(("not", ("not", (3, "found"))))) == (3, _lib.PRED_FOUND, 0, 0, 0)
    assert fields(made((2, "type", "object"))) == (2, _lib.PRED_TYPE, 0, 0, 1)
    assert fields(made((2, "type", ["number", "null"]))) == (2, _lib.PRED_TYPE, 0, 0, 8 | 16 | 128)
    assert fields(made((1, ">", 250))) == (1, _lib.PRED_NUM_GT, 0, 0, 250)
    assert fields(made((1, "<=", -1))) == (1, _lib.PRED_NUM_LE, 0, 0, 0xFFFFFFFFFFFFFFFF)
    assert fields(made((1, "==", 250.5))) == (1, _lib.PRED_NUM_EQ, _lib.PRED_DOUBLE, 0, struct.unpack("<Q", struct.pack("<d", 250.5))[0])
    for spec, op, data in (((0, "==", "error"), _lib.PRED_STR_EQ, b"error"), ((0, "prefix", b"a\0b"), _lib.PRED_STR_PREFIX, b"a\0b"),
                           ((15, "==", "é"), _lib.PRED_STR_EQ, "é".encode()), ((0, "==", ""), _lib.PRED_STR_EQ, b"")):
        p = made(spec)
        assert fields(p) == (spec[0], op, 0, len(data), 0) and ctypes.string_at(p.operand_bytes, len(data)) == data
    # the twin's compile step takes them all, as msj_predicates_create does
    ftwin = tfm.load_twin()
    specs = [(0, "found"), ("not", (1, ">=", 2**63 - 1)), (2, "type", "bool"), (3, "prefix", "x" * 255), (4, "<", 1e308)]
    table = (_lib.MsjPredicate * len(specs))(*[made(s) for s in specs])
    blob = ctypes.create_string_buffer(ftwin.frm_predicates_bytes())
    assert ftwin.frm_compile(table, len(specs), _lib.PREDICATES_ANY, blob) == 0


@pytest.mark.parametrize("spec", [(0, "==", True), (0, ">", False), (0, "type", "thing"), (0, "type", []), (0, "found", 1), (0, "~", 1), (0, "prefix", 5),
                                  (0, ">", "5"), (0, "==", None), (0, "==", 2**63), (-1, "found"), ("/a", "found"), (True, "found"), (0,), (0, 1, 2),
                                  (0, "==", 1, 2), ("not", (0, "==", True))])
def test_specs_that_are_none(spec):
    with pytest.raises(ValueError):
        predicate_struct(spec, [])


def test_columns_by_name():
    index = ["", "/status", "/latency"].index
    assert _column_specs([("/status", "==", "error"), ("not", ("/latency", ">", 250.5)), ["", "found"]], index) == \
        [(1, "==", "error"), ("not", (2, ">", 250.5)), (0, "found")]
    with pytest.raises(ValueError):
        _column_specs([("/nowhere", "found")], index)
