"""A host-side view of the document that ``msj_tape_device`` builds (include/msj_stage1.h): the tape and the string buffer.

The layout is the reference's ``Document`` (include/dom/document.mojo): ``tape`` is a list of 64-bit words, the type in
the top byte and a 56-bit payload below; ``string_buf`` holds one record per string, a 4-byte little-endian length and
the bytes.  This module only reads what the kernels wrote: numpy arrays, no device code.
"""
import struct

import numpy as np

VALUE_MASK = (1 << 56) - 1
COUNT_MASK = 0xFFFFFF


class Document:
    """``tape``: numpy uint64[tape_words]; ``string_buf``: numpy uint8[string_bytes]."""

    def __init__(self, tape, string_buf):
        self.tape = np.ascontiguousarray(tape, dtype=np.uint64)
        self.string_buf = np.ascontiguousarray(string_buf, dtype=np.uint8)

    @classmethod
    def from_device(cls, tape_result, d_tape, d_string_buf):
        """From what ``Stage1Device.tape`` / ``parse_document`` returned (code 0): copies the used parts to the host."""
        if tape_result.code != 0:
            raise ValueError(f"no document: msj_tape_device code {tape_result.code}")
        tape = d_tape[:int(tape_result.tape_words)].cpu().numpy().view(np.uint64)
        sbuf = d_string_buf[:int(tape_result.string_bytes)].cpu().numpy()
        return cls(tape, sbuf)

    def string_at(self, offset):
        """The bytes of the string record at `offset` of the string buffer."""
        offset = int(offset)
        (n,) = struct.unpack_from("<I", self.string_buf, offset)
        return self.string_buf[offset + 4:offset + 4 + n].tobytes()

    def dump_raw_tape(self):
        """The reference's ``dump_raw_tape`` (include/dom/document.mojo:54-169), the same text line for line: -> (text,
        ok).  One departure: the reference takes the word count from tape[1]; it is read from tape[0] here, where
        visit_document_end writes it, and the last root word is printed after the loop as the reference does."""
        tape = self.tape
        out = []
        if tape.size < 2 or int(tape[0]) >> 56 != ord("r"):
            return "", False
        how_many = int(tape[0]) & VALUE_MASK
        out.append(f"0 : {ord('r')}\t// pointing to {how_many} (right after last node)\n")
        if how_many > tape.size:
            return "".join(out), False
        i = 1
        while i < how_many - 1:
            w = int(tape[i])
            t, payload = w >> 56, w & VALUE_MASK
            line = f"{i} : "
            if t == ord('"'):
                line += 'string "' + self.string_at(payload).decode("utf-8", errors="replace") + '"\n'
            elif t in (ord("l"), ord("u"), ord("d")):
                if i + 1 >= how_many:
                    return "".join(out), False
                i += 1
                v = int(tape[i])
                if t == ord("l"):
                    line += f"integer {v - (1 << 64) if v >> 63 else v}\n"
                elif t == ord("u"):
                    line += f"unsigned integer {v}\n"
                else:
                    line += f"float {struct.unpack('<d', struct.pack('<Q', v))[0]}\n"
            elif t == ord("n"):
                line += "null\n"
            elif t == ord("t"):
                line += "true\n"
            elif t == ord("f"):
                line += "false\n"
            elif t in (ord("{"), ord("[")):
                line += f"{chr(t)}\t// pointing to next tape location {payload & 0xFFFFFFFF} (first node after the scope), " \
                        f" saturated count {(payload >> 32) & COUNT_MASK}\n"
            elif t in (ord("}"), ord("]")):
                line += f"{chr(t)}\t// pointing to previous tape location {payload & 0xFFFFFFFF} (start of the scope)\n"
            else:
                return "".join(out), False
            out.append(line)
            i += 1
        w = int(tape[i])
        out.append(f"{i} : {w >> 56}\t// pointing to {w & VALUE_MASK} (start root)\n")
        return "".join(out), True

    def to_python(self):
        """The document as Python values (dict, list, str, int, float, bool, None), without recursion.  Duplicate keys: the
        last one wins, as in ``json.loads``."""
        tape = self.tape
        how_many = int(tape[0]) & VALUE_MASK
        stack = []  # [container, pending key or None]
        root = []
        cur, key = root, None
        i = 1
        while i < how_many - 1:
            w = int(tape[i])
            t, payload = w >> 56, w & VALUE_MASK
            i += 1
            if t in (ord("}"), ord("]")):
                done = cur
                cur, key = stack.pop()
                v = done
            elif t in (ord("{"), ord("[")):
                stack.append((cur, key))
                cur, key = ({} if t == ord("{") else []), None
                continue
            elif t == ord('"'):
                v = self.string_at(payload).decode("utf-8")
                if isinstance(cur, dict) and key is None:
                    key = v
                    continue
            elif t == ord("l"):
                v = int(tape[i])
                v = v - (1 << 64) if v >> 63 else v
                i += 1
            elif t == ord("u"):
                v = int(tape[i])
                i += 1
            elif t == ord("d"):
                v = struct.unpack("<d", struct.pack("<Q", int(tape[i])))[0]
                i += 1
            elif t == ord("t"):
                v = True
            elif t == ord("f"):
                v = False
            elif t == ord("n"):
                v = None
            else:
                raise ValueError(f"tape word {i - 1}: unknown type {t}")
            if isinstance(cur, dict):
                cur[key] = v
                key = None
            else:
                cur.append(v)
        if stack or len(root) != 1:
            raise ValueError("tape does not hold one document")
        return root[0]
