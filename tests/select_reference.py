"""The definition of msj_select_documents_device's lookup in Python, written from the text of include/msj_stage1.h only: a
JSON pointer of object keys looked up in one document's text.  No tokens, depths or partners: the document is decoded by
json with a hook that keeps the FIRST of duplicate keys (at_key's rule; json.loads alone would keep the last), and the
keys are walked.  tests/test_select_math.py holds the host twin of the kernels' arithmetic against it.
"""
import functools
import json

NO_SUCH_FIELD, INCORRECT_TYPE, INVALID_JSON_POINTER = 20, 17, 22
MAX_PATHS, MAX_SEGMENTS, MAX_SEGMENT_BYTES = 16, 8, 255


class Obj(dict):
    """A JSON object as the decoder built it: the first of duplicate keys kept"""


def _first_wins(pairs):
    out = Obj()
    for key, value in pairs:
        out.setdefault(key, value)
    return out


_DECODER = json.JSONDecoder(object_pairs_hook=_first_wins)


def decode(text):
    """One document's text (bytes) -> its value, the first of duplicate keys kept at every level"""
    return _DECODER.decode(text.decode("utf-8"))


def segments(pointer):
    """RFC 6901: "" -> [], "/a/b" -> ["a", "b"], ~1 -> "/", ~0 -> "~".  ValueError(22) for a pointer that is none."""
    if pointer == "":
        return []
    if not pointer.startswith("/"):
        raise ValueError(INVALID_JSON_POINTER)
    out = []
    for raw in pointer[1:].split("/"):
        seg, k = [], 0
        while k < len(raw):
            if raw[k] == "~":
                if raw[k + 1:k + 2] not in ("0", "1"):
                    raise ValueError(INVALID_JSON_POINTER)
                seg.append("~" if raw[k + 1] == "0" else "/")
                k += 2
            else:
                seg.append(raw[k])
                k += 1
        out.append("".join(seg))
    return out


@functools.lru_cache(maxsize=None)
def _segments_once(pointer):
    return tuple(segments(pointer))


def lookup(value, pointer):
    """The pointer in a decoded document (decode) -> (code, value): (0, the value), (17, None) where a segment meets
    something that is no object, (20, None) where the object has no such key"""
    for seg in _segments_once(pointer):
        if not isinstance(value, Obj):
            return INCORRECT_TYPE, None
        if seg not in value:
            return NO_SUCH_FIELD, None
        value = value[seg]
    return 0, value


def key_paths(value, prefix=(), out=None):
    """Every chain of object keys in a decoded document (through objects only, as the lookup goes) -> set of tuples"""
    out = set() if out is None else out
    if isinstance(value, Obj):
        for key, v in value.items():
            out.add(prefix + (key,))
            key_paths(v, prefix + (key,), out)
    return out


def pointer_of(keys):
    """A chain of keys as a JSON pointer"""
    return "".join("/" + k.replace("~", "~0").replace("/", "~1") for k in keys)
