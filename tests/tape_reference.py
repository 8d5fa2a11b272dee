"""A plain serial tape builder, written from the definition of msj_tape_device in include/msj_stage1.h.

A loop and a stack over the bytes and the stage-1 offsets, the way the reference's TapeBuilder walks a document: no
bracket partners, no depths, no prefix sums -- so that it shares nothing with the kernels' formulation (tape_math.h) that
tests/test_tape_math.py and tests/test_tape.py hold against it.  Only valid documents (msj_validate_device code 0) have a
tape; number values come from tests/test_number_math.expected.
"""
import struct

from tests import test_number_math as tnm

MAX_COUNT = 0xFFFFFF
SIMPLE = {0x22: 0x22, 0x5C: 0x5C, 0x2F: 0x2F, 0x62: 8, 0x66: 12, 0x6E: 10, 0x72: 13, 0x74: 9}


def word(tag, payload=0):
    return (tag << 56) | payload


def unescape(data, start):
    """The bytes of the string whose opening quote is at `start` (a valid, closed string)."""
    out = bytearray()
    p = start + 1
    while data[p] != 0x22:
        c = data[p]
        if c != 0x5C:
            out.append(c)
            p += 1
            continue
        e = data[p + 1]
        if e != 0x75:
            out.append(SIMPLE[e])
            p += 2
            continue
        cp = int(data[p + 2:p + 6], 16)
        p += 6
        if 0xD800 <= cp <= 0xDBFF:
            lo = int(data[p + 2:p + 6], 16)
            assert data[p:p + 2] == b"\\u" and 0xDC00 <= lo <= 0xDFFF
            cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00)
            p += 6
        out += chr(cp).encode("utf-8")
    return bytes(out)


def build(data, idx):
    """(tape: list of int, string_buf: bytes) of the valid document `data` with structural offsets `idx`."""
    tape = [0]
    sbuf = bytearray()
    stack = []  # [tape index of the opening word, commas]
    for s in idx:
        s = int(s)
        c = data[s]
        if c in b"{[":
            stack.append([len(tape), 0])
            tape.append(word(c))
        elif c in b"}]":
            start, commas = stack.pop()
            if len(tape) == start + 1:
                tape[start] |= start + 2  # empty_container
            else:
                tape[start] |= (min(1 + commas, MAX_COUNT) << 32) | (len(tape) + 1)
            tape.append(word(c, start))
        elif c == 0x2C:
            stack[-1][1] += 1
        elif c == 0x3A:
            pass
        elif c == 0x22:
            body = unescape(data, s)
            tape.append(word(0x22, len(sbuf)))
            sbuf += struct.pack("<I", len(body)) + body
        elif c in b"tfn":
            tape.append(word(c))
        else:
            kind, bits = tnm.expected(data, s)
            assert kind in (tnm.INT64, tnm.DOUBLE), data[s:s + 30]
            tape.append(word(ord("l") if kind == tnm.INT64 else ord("d")))
            tape.append(bits)
    assert not stack
    tape.append(word(ord("r"), 0))
    tape[0] = word(ord("r"), len(tape))
    return tape, bytes(sbuf)


def decode(tape, sbuf):
    """(tape, string buffer) back to a Python value: objects as lists of (key, value) pairs, ints from 'l', floats from the
    bit pattern of 'd'.  Checks the links on the way."""
    assert tape[0] == word(ord("r"), len(tape)) and tape[-1] == word(ord("r"), 0)

    def string_at(off):
        (n,) = struct.unpack_from("<I", sbuf, off)
        return bytes(sbuf[off + 4:off + 4 + n]).decode("utf-8")

    def value(i):
        w = int(tape[i])
        tag, payload = w >> 56, w & ((1 << 56) - 1)
        if tag == 0x22:
            return string_at(payload), i + 1
        if tag == ord("l"):
            v = int(tape[i + 1])
            return (v - (1 << 64) if v >> 63 else v), i + 2
        if tag == ord("d"):
            return struct.unpack("<d", struct.pack("<Q", int(tape[i + 1])))[0], i + 2
        if tag in b"tfn":
            return {ord("t"): True, ord("f"): False, ord("n"): None}[tag], i + 1
        assert tag in b"{[", (i, hex(w))
        after, count = payload & 0xFFFFFFFF, (payload >> 32) & MAX_COUNT
        close = int(tape[after - 1])
        assert close == word(tag + 2, i), (i, hex(w), hex(close))
        items = []
        j = i + 1
        while j < after - 1:
            if tag == ord("{"):
                assert int(tape[j]) >> 56 == 0x22
                key, j = value(j)
                v, j = value(j)
                items.append((key, v))
            else:
                v, j = value(j)
                items.append(v)
        assert j == after - 1 and count == min(len(items), MAX_COUNT), (i, count, len(items))
        return items, after

    v, end = value(1)
    assert end == len(tape) - 1
    return v


def same(a, b):
    """Equality with floats compared by bit pattern and no bool / int / float mixing."""
    if type(a) is not type(b):
        if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return False
    if isinstance(a, float):
        return struct.pack("<d", a) == struct.pack("<d", b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b
