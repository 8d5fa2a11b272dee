"""ctypes binding of ``libmsj_stage1.so`` (the C ABI in ``include/msj_stage1.h``).

The HIP extension is the only implementation behind this package: if the shared
library is missing, or no HIP device is usable, calls raise -- there is no CPU
fallback of any kind.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# The one library this package loads.  No environment variable can substitute it; measurement scripts that compare
# differently built kernels set this attribute explicitly before the first load() (bench.py --lib, which reports it).
LIB_PATH = os.path.join(_HERE, "libmsj_stage1.so")
GEN_LIB_PATH = os.path.join(_HERE, "libmsj_gen.so")


class MsjCarry(ctypes.Structure):
    """``msj_carry`` (include/msj_stage1.h): the scanners' cross-block state."""

    _fields_ = [
        ("count", ctypes.c_uint64),
        ("bytes", ctypes.c_uint64),
        ("in_string", ctypes.c_uint32),
        ("next_is_escaped", ctypes.c_uint32),
        ("prev_scalar", ctypes.c_uint32),
        ("unescaped_error", ctypes.c_uint32),
        ("utf8_error", ctypes.c_uint32),
        ("internal_error", ctypes.c_uint32),
        ("code", ctypes.c_int32),
        ("capacity_error", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32 * 4),
    ]


class MsjTokensResult(ctypes.Structure):
    """``msj_tokens_result`` (include/msj_stage1.h)."""

    _fields_ = [("n", ctypes.c_uint64), ("final_depth", ctypes.c_int32), ("min_depth", ctypes.c_int32),
                ("max_depth", ctypes.c_int32), ("reserved", ctypes.c_uint32)]


class MsjDocumentsResult(ctypes.Structure):
    """``msj_documents_result`` (include/msj_stage1.h)."""

    _fields_ = [("n_documents", ctypes.c_uint64), ("n_complete", ctypes.c_uint64),
                ("tokens_complete", ctypes.c_uint64), ("resume_offset", ctypes.c_uint64)]


class MsjNumber(ctypes.Structure):
    """``msj_number`` (include/msj_stage1.h): one record per number token, in token order."""

    _fields_ = [("bits", ctypes.c_uint64), ("token", ctypes.c_uint32), ("kind", ctypes.c_uint32)]


class MsjNumbersResult(ctypes.Structure):
    """``msj_numbers_result`` (include/msj_stage1.h)."""

    _fields_ = [("n_numbers", ctypes.c_uint64), ("n_errors", ctypes.c_uint64), ("first_error", ctypes.c_uint64),
                ("n_slow", ctypes.c_uint64)]


NUMBER_INT64, NUMBER_DOUBLE, NUMBER_ERR_SYNTAX, NUMBER_ERR_RANGE = 1, 2, 3, 4


class MsjValidateResult(ctypes.Structure):
    """``msj_validate_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("error_token", ctypes.c_uint64),
                ("error_offset", ctypes.c_uint64), ("n_escaped", ctypes.c_uint64)]


VALIDATE_NUMBERS_UNCHECKED, VALIDATE_COUNTS_CLIPPED, VALIDATE_BIG_CONTAINERS = 1, 2, 64


class MsjDocumentVerdict(ctypes.Structure):
    """``msj_document_verdict`` (include/msj_stage1.h): one per complete document of a window."""

    _fields_ = [("code", ctypes.c_int32), ("reserved", ctypes.c_uint32), ("error_token", ctypes.c_uint64)]


class MsjValidateDocumentsResult(ctypes.Structure):
    """``msj_validate_documents_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_documents", ctypes.c_uint64),
                ("n_invalid", ctypes.c_uint64), ("first_invalid", ctypes.c_uint64), ("n_escaped", ctypes.c_uint64),
                ("reserved", ctypes.c_uint64)]


class MsjTapeResult(ctypes.Structure):
    """``msj_tape_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("tape_words", ctypes.c_uint64),
                ("string_bytes", ctypes.c_uint64), ("n_strings", ctypes.c_uint64)]


class MsjDocumentTape(ctypes.Structure):
    """``msj_document_tape`` (include/msj_stage1.h): one per complete document of a window."""

    _fields_ = [("tape_first", ctypes.c_uint64), ("string_first", ctypes.c_uint64), ("tape_words", ctypes.c_uint32),
                ("code", ctypes.c_int32), ("string_bytes", ctypes.c_uint64)]


class MsjTapeDocumentsResult(ctypes.Structure):
    """``msj_tape_documents_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_documents", ctypes.c_uint64),
                ("n_built", ctypes.c_uint64), ("tape_words", ctypes.c_uint64), ("string_bytes", ctypes.c_uint64),
                ("n_strings", ctypes.c_uint64), ("n_numbers", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


class MsjField(ctypes.Structure):
    """``msj_field`` (include/msj_stage1.h): one per (path, document) of a window."""

    _fields_ = [("bits", ctypes.c_uint64), ("token", ctypes.c_uint32), ("type", ctypes.c_uint8), ("flags", ctypes.c_uint8),
                ("code", ctypes.c_uint16)]


class MsjSelectDocumentsResult(ctypes.Structure):
    """``msj_select_documents_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_documents", ctypes.c_uint64),
                ("n_paths", ctypes.c_uint64), ("n_found", ctypes.c_uint64), ("n_no_bits", ctypes.c_uint64),
                ("reserved", ctypes.c_uint64)]


class MsjStringColumnResult(ctypes.Structure):
    """``msj_string_column_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_strings", ctypes.c_uint64),
                ("n_escaped", ctypes.c_uint64), ("total_bytes", ctypes.c_uint64), ("n_other", ctypes.c_uint64)]


class MsjArrayColumnResult(ctypes.Structure):
    """``msj_array_column_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_arrays", ctypes.c_uint64),
                ("n_elements", ctypes.c_uint64), ("n_other", ctypes.c_uint64), ("n_no_bits", ctypes.c_uint64)]


class MsjObjectEntriesResult(ctypes.Structure):
    """``msj_object_entries_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_objects", ctypes.c_uint64),
                ("n_entries", ctypes.c_uint64), ("n_other", ctypes.c_uint64), ("n_no_bits", ctypes.c_uint64)]


class MsjRawColumnResult(ctypes.Structure):
    """``msj_raw_column_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_values", ctypes.c_uint64),
                ("n_containers", ctypes.c_uint64), ("total_bytes", ctypes.c_uint64), ("n_other", ctypes.c_uint64)]


class MsjDictionaryResult(ctypes.Structure):
    """``msj_dictionary_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_values", ctypes.c_uint64),
                ("n_distinct", ctypes.c_uint64), ("dict_bytes", ctypes.c_uint64), ("max_probe", ctypes.c_uint64)]


class MsjDictionaryExtendResult(ctypes.Structure):
    """``msj_dictionary_extend_result`` (include/msj_stage1.h): ``msj_dictionary_result``'s members, then two more."""

    _fields_ = MsjDictionaryResult._fields_ + [("n_prior", ctypes.c_uint64), ("n_matched", ctypes.c_uint64)]


class MsjPredicate(ctypes.Structure):
    """``msj_predicate`` (include/msj_stage1.h)."""

    _fields_ = [("column", ctypes.c_uint32), ("op", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("operand_len", ctypes.c_uint32),
                ("operand_bits", ctypes.c_uint64), ("operand_bytes", ctypes.c_void_p)]


class MsjFilterRowsResult(ctypes.Structure):
    """``msj_filter_rows_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_kept", ctypes.c_uint64),
                ("n_no_bits", ctypes.c_uint64), ("n_missing", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


class MsjTakeRowsResult(ctypes.Structure):
    """``msj_take_rows_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_out_of_range", ctypes.c_uint64),
                ("n_found", ctypes.c_uint64), ("n_no_bits", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


class MsjCastStringsResult(ctypes.Structure):
    """``msj_cast_strings_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_cast", ctypes.c_uint64),
                ("n_syntax", ctypes.c_uint64), ("n_range", ctypes.c_uint64), ("n_other", ctypes.c_uint64)]


class MsjAggregate(ctypes.Structure):
    """``msj_aggregate`` (include/msj_stage1.h): the record of one (column, group)."""

    _fields_ = [("n_rows", ctypes.c_uint64), ("n_values", ctypes.c_uint64), ("sum_bits", ctypes.c_uint64), ("min_bits", ctypes.c_uint64),
                ("max_bits", ctypes.c_uint64), ("sum_type", ctypes.c_uint8), ("min_type", ctypes.c_uint8), ("max_type", ctypes.c_uint8),
                ("flags", ctypes.c_uint8), ("reserved", ctypes.c_uint32)]


class MsjAggregateResult(ctypes.Structure):
    """``msj_aggregate_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_groups", ctypes.c_uint64),
                ("n_ungrouped", ctypes.c_uint64), ("n_values", ctypes.c_uint64), ("n_skipped", ctypes.c_uint64)]


# msj_aggregate.flags; the most groups msj_debug_set_aggregate_limits takes
AGG_INT_OVERFLOW, AGG_INFINITE = 1, 2
AGG_MAX_LDS_GROUPS = 256

class MsjSortRowsResult(ctypes.Structure):
    """``msj_sort_rows_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_values", ctypes.c_uint64),
                ("n_written", ctypes.c_uint64), ("n_skipped", ctypes.c_uint64), ("n_out_of_range", ctypes.c_uint64)]


# msj_sort_rows_device: flags; msj_debug_set_sort_mode
SORT_DESCENDING, SORT_VALUES_ONLY = 1, 2
SORT_MODE_AUTO, SORT_MODE_FULL, SORT_MODE_SELECT = 0, 1, 2

class MsjJoinRowsResult(ctypes.Structure):
    """``msj_join_rows_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_left", ctypes.c_uint64), ("n_right", ctypes.c_uint64),
                ("n_keys", ctypes.c_uint64), ("n_pairs", ctypes.c_uint64), ("n_left_matched", ctypes.c_uint64),
                ("n_left_null", ctypes.c_uint64), ("n_right_null", ctypes.c_uint64)]


# msj_join_rows_device: the kind (flags & 3); the right side of a pair without one
JOIN_INNER, JOIN_LEFT, JOIN_SEMI, JOIN_ANTI = 0, 1, 2, 3
JOIN_KINDS = {"inner": JOIN_INNER, "left": JOIN_LEFT, "semi": JOIN_SEMI, "anti": JOIN_ANTI}
JOIN_NO_ROW = 0xFFFFFFFF

class MsjDictionaryOrderResult(ctypes.Structure):
    """``msj_dictionary_order_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_entries", ctypes.c_uint64), ("n_values", ctypes.c_uint64),
                ("n_tied", ctypes.c_uint64), ("depth", ctypes.c_uint64), ("n_equal", ctypes.c_uint64)]


class MsjRankRowsResult(ctypes.Structure):
    """``msj_rank_rows_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_ranked", ctypes.c_uint64),
                ("n_null", ctypes.c_uint64), ("n_unknown", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


class MsjPattern(ctypes.Structure):
    """``msj_pattern`` (include/msj_stage1.h): the pieces back to back, their number, the flags, their lengths."""

    _fields_ = [("bytes", ctypes.c_void_p), ("n_pieces", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("piece_len", ctypes.c_uint32 * 4)]


class MsjMatchStringsResult(ctypes.Structure):
    """``msj_match_strings_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_values", ctypes.c_uint64),
                ("n_matched", ctypes.c_uint64), ("max_pieces", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


class MsjKeyPart(ctypes.Structure):
    """``msj_key_part`` (include/msj_stage1.h): one column of a group key -- a host array."""

    _fields_ = [("d_column", ctypes.c_void_p), ("kind", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class MsjBucketRowsResult(ctypes.Structure):
    """``msj_bucket_rows_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_bucketed", ctypes.c_uint64),
                ("n_range", ctypes.c_uint64), ("n_skipped", ctypes.c_uint64), ("n_other", ctypes.c_uint64)]


class MsjGroupKeysResult(ctypes.Structure):
    """``msj_group_keys_result`` (include/msj_stage1.h)."""

    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_keys", ctypes.c_uint64),
                ("n_null_rows", ctypes.c_uint64), ("key_width", ctypes.c_uint64), ("bytes_len", ctypes.c_uint64)]


# msj_key_part.kind and .flags, the bytes of a part by kind, the most parts and the widest key
KEY_NUMBER, KEY_CODE = 1, 2
KEY_KINDS = {"number": KEY_NUMBER, "code": KEY_CODE}
KEY_NULL_IS_GROUP = 1
KEY_PART_BYTES = {KEY_NUMBER: 11, KEY_CODE: 5}
KEY_MAX_PARTS, KEY_MAX_WIDTH = 8, 88

# msj_pattern.flags; the limits of msj_patterns_create
MATCH_AT_START, MATCH_AT_END, MATCH_NOCASE_ASCII = 1, 2, 4
MATCH_FLAGS = {"at_start": MATCH_AT_START, "at_end": MATCH_AT_END, "nocase": MATCH_NOCASE_ASCII}
MATCH_MAX_PATTERNS, MATCH_MAX_PIECES, MATCH_MAX_PIECE_BYTES = 16, 4, 255

# msj_dictionary_order_device: flags, the rank of an entry without a value, the most rounds; msj_debug_set_order_mode
ORDER_CONTINUE = 1
ORDER_NO_RANK = 0xFFFFFFFF
ORDER_MAX_ROUNDS = 64
ORDER_DEFAULT_ROUNDS_GROUP, ORDER_DEFAULT_ROUNDS_GRID, ORDER_GROUP_ENTRIES = 64, 4, 1024
ORDER_MODE_AUTO, ORDER_MODE_GRID, ORDER_MODE_GROUP = 0, 1, 2

# msj_cast_strings_device: kind, unit, flags; msj_debug_set_cast_fetch
CAST_TIMESTAMP, CAST_NUMBER = 1, 2
CAST_KINDS = {"timestamp": CAST_TIMESTAMP, "number": CAST_NUMBER}
CAST_UNITS = {"s": 0, "ms": 1, "us": 2, "ns": 3}
CAST_UNIT_PER_SECOND = {"s": 1, "ms": 10**3, "us": 10**6, "ns": 10**9}
CAST_KEEP_NUMBERS = 1
CAST_FETCH_WINDOW, CAST_FETCH_BYTES = 0, 1

# msj_predicate.op, .flags, msj_predicates_create's flags, MSJ_PRED_TYPE's mask bits by tape tag
PRED_FOUND, PRED_TYPE, PRED_NUM_EQ, PRED_NUM_LT, PRED_NUM_LE, PRED_NUM_GT, PRED_NUM_GE, PRED_STR_EQ, PRED_STR_PREFIX = range(9)
PRED_NOT, PRED_DOUBLE, PREDICATES_ANY = 1, 2, 1
TYPE_BITS = {"{": 1, "[": 2, '"': 4, "l": 8, "d": 16, "t": 32, "f": 64, "n": 128}
MAX_PREDICATES, MAX_COLUMNS, MAX_OPERAND_BYTES = 16, 16, 255

RAW_COMPACT = 1   # MSJ_RAW_COMPACT
DICTIONARY_WEAK_HASH = 1   # MSJ_DICTIONARY_WEAK_HASH (a test aid)
DICTIONARY_FROZEN = 2      # MSJ_DICTIONARY_FROZEN (msj_dictionary_extend_device: look up only)
DICTIONARY_NO_ENTRY = -2   # ... the code of a row whose value the frozen dictionary does not hold
FIELD_NO_BITS = 64
NO_SUCH_FIELD, INCORRECT_TYPE, INVALID_JSON_POINTER = 20, 17, 22
MAX_PATHS, MAX_PATH_SEGMENTS, MAX_SEGMENT_BYTES = 16, 8, 255


class MsjSegment(ctypes.Structure):
    _fields_ = [
        ("byte_base", ctypes.c_uint64),
        ("byte_len", ctypes.c_uint64),
        ("index_begin", ctypes.c_uint64),
        ("count", ctypes.c_uint64),
    ]


assert ctypes.sizeof(MsjCarry) == 64
assert ctypes.sizeof(MsjSegment) == 32
assert ctypes.sizeof(MsjNumber) == 16 and ctypes.sizeof(MsjNumbersResult) == 32
assert ctypes.sizeof(MsjValidateResult) == 32
assert ctypes.sizeof(MsjTapeResult) == 32
assert ctypes.sizeof(MsjDocumentVerdict) == 16 and ctypes.sizeof(MsjValidateDocumentsResult) == 48

assert ctypes.sizeof(MsjDocumentTape) == 32 and ctypes.sizeof(MsjTapeDocumentsResult) == 64
assert ctypes.sizeof(MsjField) == 16 and ctypes.sizeof(MsjSelectDocumentsResult) == 48
assert ctypes.sizeof(MsjPattern) == 32 and ctypes.sizeof(MsjMatchStringsResult) == 48
assert ctypes.sizeof(MsjKeyPart) == 16 and ctypes.sizeof(MsjBucketRowsResult) == 48 and ctypes.sizeof(MsjGroupKeysResult) == 48
assert ctypes.sizeof(MsjStringColumnResult) == 48 and ctypes.sizeof(MsjArrayColumnResult) == 48
assert ctypes.sizeof(MsjObjectEntriesResult) == 48 and ctypes.sizeof(MsjRawColumnResult) == 48
assert ctypes.sizeof(MsjDictionaryResult) == 48 and ctypes.sizeof(MsjDictionaryExtendResult) == 64

_lib = None


class HipExtensionMissing(RuntimeError):
    pass


def _share_torch_hip_runtime():
    """Make libmsj_stage1.so bind to the HIP runtime PyTorch already uses.

    The PyTorch wheel bundles its own libamdhip64.so / libhsa-runtime64.so
    (ROCm 7.0) next to the system ROCm 7.2 that libmsj_stage1.so names in its
    DT_NEEDED.  Two HIP runtimes in one process each open the device; whichever
    comes second may see no GPU, and tensors allocated by one are unknown to the
    other.  Promoting torch's runtime to the global symbol scope *before* our
    library is opened makes every hip* symbol of libmsj_stage1.so resolve to
    that one runtime (global scope is searched before a library's own
    dependencies).  Without torch in the process (the Mojo shim case) nothing is
    preloaded and the system runtime is used.
    """
    try:
        import torch  # noqa: F401
    except ImportError:
        return
    cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)


def load():
    """Load libmsj_stage1.so once; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    _share_torch_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise HipExtensionMissing(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C mojo_simdjson_amd/csrc)"
        )
    lib = ctypes.CDLL(LIB_PATH)
    u8p, u32p, u64p = ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)
    i32p = ctypes.POINTER(ctypes.c_int32)
    lib.msj_version.restype = ctypes.c_char_p
    lib.msj_version.argtypes = []
    lib.msj_device_count.restype = ctypes.c_int32
    lib.msj_device_count.argtypes = []
    lib.msj_tile_bytes.restype = ctypes.c_uint32
    lib.msj_tile_bytes.argtypes = []
    lib.msj_ctx_create.restype = ctypes.c_int32
    lib.msj_ctx_create.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]
    lib.msj_ctx_destroy.restype = None
    lib.msj_ctx_destroy.argtypes = [ctypes.c_void_p]
    lib.msj_stage1.restype = ctypes.c_int32
    lib.msj_stage1.argtypes = [u8p, ctypes.c_uint64, u32p, ctypes.c_uint64, u64p, i32p, ctypes.c_uint32]
    lib.msj_stage1_ctx.restype = ctypes.c_int32
    lib.msj_stage1_ctx.argtypes = [ctypes.c_void_p] + lib.msj_stage1.argtypes
    lib.msj_stage1_device.restype = ctypes.c_int32
    lib.msj_stage1_device.argtypes = [
        ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_uint32,
    ]
    lib.msj_tokens_device.restype = ctypes.c_int32
    lib.msj_tokens_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p]
    lib.msj_token_spans_device.restype = ctypes.c_int32
    lib.msj_token_spans_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_stage2_prep_device.restype = ctypes.c_int32
    lib.msj_stage2_prep_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64] + [ctypes.c_void_p] * 7
    lib.msj_tokens_chain_device.restype = ctypes.c_int32
    lib.msj_tokens_chain_device.argtypes = lib.msj_tokens_device.argtypes[:-1] + [ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_stage2_prep_chain_device.restype = ctypes.c_int32
    lib.msj_stage2_prep_chain_device.argtypes = lib.msj_stage2_prep_device.argtypes[:-1] + [ctypes.c_void_p, ctypes.c_void_p]
    # (round 5) the pairs form, the types prototype, the placement report: every 64-bit argument declared -- an undeclared
    # Python int goes over as a C int, and a buffer length over 2 GiB arrived truncated (found by the 3.94 GiB pairs test)
    lib.msj_stage2_prep_pairs_device.restype = ctypes.c_int32
    lib.msj_stage2_prep_pairs_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64] + [ctypes.c_void_p] * 8
    lib.msj_tokens_pairs_device.restype = ctypes.c_int32
    lib.msj_tokens_pairs_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64] + [ctypes.c_void_p] * 6
    lib.msj_stage1_types_device.restype = ctypes.c_int32
    lib.msj_stage1_types_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_uint32]
    lib.msj_depth_from_types_device.restype = ctypes.c_int32
    lib.msj_depth_from_types_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64] + [ctypes.c_void_p] * 5
    lib.msj_host_placement.restype = ctypes.c_int32
    lib.msj_host_placement.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64]
    lib.msj_debug_numa_node_of.restype = ctypes.c_int32
    lib.msj_debug_numa_node_of.argtypes = [ctypes.c_void_p]
    lib.msj_stage2_prep_segments.restype = ctypes.c_int32
    lib.msj_stage2_prep_segments.argtypes = [ctypes.c_void_p, u8p, ctypes.c_void_p, ctypes.c_uint32, u32p] + [ctypes.c_void_p] * 7 + \
        [ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    lib.msj_documents_device.restype = ctypes.c_int32
    lib.msj_documents_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64, ctypes.c_int32, u32p, ctypes.c_uint64,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_number_values_device.restype = ctypes.c_int32
    lib.msj_number_values_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_number_values_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_number_values_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.msj_validate_device.restype = ctypes.c_int32
    lib.msj_validate_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64] + [ctypes.c_void_p] * 6 + \
        [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_validate_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_validate_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.msj_validate_documents_device.restype = ctypes.c_int32
    lib.msj_validate_documents_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64] + [ctypes.c_void_p] * 8 + \
        [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_validate_documents_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_validate_documents_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    lib.msj_tape_device.restype = ctypes.c_int32
    lib.msj_tape_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64] + [ctypes.c_void_p] * 6 + \
        [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
         ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_tape_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_tape_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.msj_tape_documents_device.restype = ctypes.c_int32
    lib.msj_tape_documents_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64] + [ctypes.c_void_p] * 8 + \
        [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
         ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_tape_documents_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_tape_documents_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    lib.msj_paths_create.restype = ctypes.c_int32
    lib.msj_paths_create.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]
    lib.msj_paths_destroy.restype = None
    lib.msj_paths_destroy.argtypes = [ctypes.c_void_p]
    lib.msj_select_documents_device.restype = ctypes.c_int32
    lib.msj_select_documents_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64] + \
        [ctypes.c_void_p] * 8 + [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                 ctypes.c_void_p]
    lib.msj_select_documents_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_select_documents_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
    lib.msj_string_column_device.restype = ctypes.c_int32
    lib.msj_string_column_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_void_p]
    lib.msj_string_column_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_string_column_workspace_bytes.argtypes = [ctypes.c_uint64]
    lib.msj_array_column_device.restype = ctypes.c_int32
    lib.msj_array_column_device.argtypes = [ctypes.c_void_p, u32p, ctypes.c_uint64] + [ctypes.c_void_p] * 8 + \
        [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
         ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_array_column_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_array_column_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.msj_select_elements_device.restype = ctypes.c_int32
    lib.msj_select_elements_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64] + \
        [ctypes.c_void_p] * 6 + [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                 ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_select_elements_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_select_elements_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
    lib.msj_array_elements_device.restype = ctypes.c_int32
    lib.msj_array_elements_device.argtypes = [ctypes.c_void_p, u32p, ctypes.c_uint64] + [ctypes.c_void_p] * 6 + \
        [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
         ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_array_elements_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_array_elements_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.msj_object_entries_device.restype = ctypes.c_int32
    lib.msj_object_entries_device.argtypes = [ctypes.c_void_p, u32p, ctypes.c_uint64] + [ctypes.c_void_p] * 6 + \
        [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_object_entries_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_object_entries_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.msj_raw_column_device.restype = ctypes.c_int32
    lib.msj_raw_column_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64] + [ctypes.c_void_p] * 8 + \
        [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_raw_column_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_raw_column_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
    lib.msj_dictionary_device.restype = ctypes.c_int32
    lib.msj_dictionary_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                          ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_dictionary_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_dictionary_workspace_bytes.argtypes = [ctypes.c_uint64]
    lib.msj_dictionary_extend_device.restype = ctypes.c_int32
    lib.msj_dictionary_extend_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_dictionary_extend_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_dictionary_extend_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.msj_predicates_create.restype = ctypes.c_int32
    lib.msj_predicates_create.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]
    lib.msj_predicates_destroy.restype = None
    lib.msj_predicates_destroy.argtypes = [ctypes.c_void_p]
    lib.msj_filter_rows_device.restype = ctypes.c_int32
    lib.msj_filter_rows_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                           ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                           ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_take_rows_device.restype = ctypes.c_int32
    lib.msj_take_rows_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]
    lib.msj_filter_rows_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_filter_rows_workspace_bytes.argtypes = [ctypes.c_uint64]
    lib.msj_cast_strings_device.restype = ctypes.c_int32
    lib.msj_cast_strings_device.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                            ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_cast_strings_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_cast_strings_workspace_bytes.argtypes = [ctypes.c_uint64]
    lib.msj_debug_set_cast_fetch.restype = ctypes.c_int32
    lib.msj_debug_set_cast_fetch.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    lib.msj_aggregate_device.restype = ctypes.c_int32
    lib.msj_aggregate_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_aggregate_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_aggregate_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
    lib.msj_debug_set_aggregate_limits.restype = ctypes.c_int32
    lib.msj_debug_set_aggregate_limits.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    lib.msj_sort_rows_device.restype = ctypes.c_int32
    lib.msj_sort_rows_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]
    lib.msj_sort_rows_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_sort_rows_workspace_bytes.argtypes = [ctypes.c_uint64]
    lib.msj_debug_set_sort_mode.restype = ctypes.c_int32
    lib.msj_debug_set_sort_mode.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    lib.msj_join_rows_device.restype = ctypes.c_int32
    lib.msj_join_rows_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                         ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]
    lib.msj_join_rows_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_join_rows_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    lib.msj_dictionary_order_device.restype = ctypes.c_int32
    lib.msj_dictionary_order_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                                ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_dictionary_order_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_dictionary_order_workspace_bytes.argtypes = [ctypes.c_uint64]
    lib.msj_debug_set_order_mode.restype = ctypes.c_int32
    lib.msj_debug_set_order_mode.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    lib.msj_rank_rows_device.restype = ctypes.c_int32
    lib.msj_rank_rows_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_patterns_create.restype = ctypes.c_int32
    lib.msj_patterns_create.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]
    lib.msj_patterns_destroy.restype = None
    lib.msj_patterns_destroy.argtypes = [ctypes.c_void_p]
    lib.msj_match_strings_device.restype = ctypes.c_int32
    lib.msj_match_strings_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p]
    lib.msj_match_strings_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_match_strings_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    lib.msj_bucket_rows_device.restype = ctypes.c_int32
    lib.msj_bucket_rows_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint32,
                                           ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_bucket_rows_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_bucket_rows_workspace_bytes.argtypes = [ctypes.c_uint64]
    lib.msj_group_keys_device.restype = ctypes.c_int32
    lib.msj_group_keys_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_group_keys_workspace_bytes.restype = ctypes.c_uint64
    lib.msj_group_keys_workspace_bytes.argtypes = [ctypes.c_uint64]
    lib.msj_carry_fetch.restype = ctypes.c_int32
    lib.msj_carry_fetch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(MsjCarry), ctypes.c_void_p]
    lib.msj_debug_set_wait_ticks.restype = ctypes.c_int32
    lib.msj_debug_set_wait_ticks.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    lib.msj_host_register.restype = ctypes.c_int32
    lib.msj_host_register.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    lib.msj_host_unregister.restype = ctypes.c_int32
    lib.msj_host_unregister.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.msj_debug_set_pipeline_min_bytes.restype = ctypes.c_int32
    lib.msj_debug_set_pipeline_min_bytes.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    lib.msj_debug_fail_pipeline_setup.restype = ctypes.c_int32
    lib.msj_debug_fail_pipeline_setup.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.msj_debug_set_span_limits.restype = ctypes.c_int32
    lib.msj_debug_set_span_limits.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
    lib.msj_debug_set_span_mode.restype = ctypes.c_int32
    lib.msj_debug_set_span_mode.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    lib.msj_debug_tile_group.restype = ctypes.c_uint32
    lib.msj_debug_tile_group.argtypes = [ctypes.c_int32]
    lib.msj_fallback_count.restype = ctypes.c_uint64
    lib.msj_fallback_count.argtypes = [ctypes.c_void_p]
    lib.msj_stage1_shard_device.restype = ctypes.c_int32
    lib.msj_stage1_shard_device.argtypes = [
        ctypes.c_void_p, u8p, ctypes.c_uint64, u32p, ctypes.c_uint64, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
        ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p,
        ctypes.c_uint32,
    ]
    _lib = lib
    return lib


def load_gen():
    if not os.path.exists(GEN_LIB_PATH):
        raise HipExtensionMissing(f"{GEN_LIB_PATH} not found: run __graft_entry__.build()")
    g = ctypes.CDLL(GEN_LIB_PATH)
    g.msj_gen_unit.restype = ctypes.c_uint64
    g.msj_gen_unit.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                               ctypes.c_int, ctypes.c_int, ctypes.c_int]
    g.msj_gen_extreme.restype = ctypes.c_uint64
    g.msj_gen_extreme.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]
    return g
