"""Documents nobody wrote by hand, and what the product must say about them: the seeded generator and the plain-Python model
of tests/test_query_fuzz_cpu.py (the host twins) and tests/test_query_fuzz.py (``DocumentStream`` on the device).

The generator writes NDJSON-like streams with its own serialiser: shuffled, absent, duplicated and escaped keys, five
whitespace styles, three separators, the same string under different bytes, numbers at the edges of int64 and binary64,
timestamps and numbers in strings, lists, maps, roots that are no object, and invalid documents that only stage 2's verdict
notices.  The field names are those of tests/stream_order.py.

The model takes its rules from the prose of include/msj_stage1.h and the docstrings of mojo_simdjson_amd/document_stream.py
and from nothing else: no ``*_math.h``, no twin, no oracle.  It uses ``json``, ``fractions``, ``datetime``, ``struct`` and
``re`` only.  A value is a span of its document's text (``Node``), found with a scanner of a few lines; every view is a list
comprehension over such spans.  There is no test in this file."""
import collections
import datetime
import json
import random
import re
import struct
from fractions import Fraction

INVALID = type("Invalid", (), {"__repr__": lambda self: "INVALID"})()
MAX_DEPTH = 100                    # DocumentStream's and tests/stream_order.py's
NUMERIC_POINTERS = ["/latency", "/ts", "/price", "/id"]
# a pointer through an array index (a numeric segment is an object key: msj_select_documents_device, "Paths"), an escaped
# pointer segment, a nested key, the empty key
EXTRA_POINTERS = ["/items/0/sku", "/attrs/a~1b", "/geo/lat", "/attrs/"]
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1

STATUS = ["active", "", "actíve", 'a"b\\c/d\n', "shared-prefix-of-a-status-value-0123456789-A", "shared-prefix-of-a-status-value-0123456789-B",
          "ok \U0001F600", "closed"]
# "sum, 'd'" of msj_aggregate (include/msj_stage1.h): the sum is the exact rational sum rounded once while every value of a
# group is a multiple of 2^(E - 95), E the largest floor(log2|v|) of the group.  The summed fields (latency, price, q) stay
# at |v| < 2^64 and on the grid of 2^-32, which satisfies that for every group a test can form; ``summable`` asserts it.
SUM_GRID = Fraction(1, 1 << 32)
LATENCY = ["0", "7", "250", "-3", "41", "-0", "9223372036854775807", "-9223372036854775808", "9007199254740993", "9007199254740992",
           "9007199254740992.0", "9007199254740994.0", "1.5", "2.5e3", "1E2", "-7.75", "0.0009765625", "-0.0", "0.0", "3.0", "3",
           "1e1", "250.0"]
UNSUMMED = ["1e308", "-1e308", "5e-324", "1.23456789012345678901234567890e5", "0.000000000000000000000000000001",
            "123456789012345678901234567890.0", "1e-400", "-1e-400", "2.2250738585072011e-308"]
TS_OTHER = ["yesterday", "", "2023-02-29T00:00:00Z", "2024-05-01T24:00:00Z", "2024-05-01T12:00:60Z", "2024-05-01T12:00", "2024-05-01",
            "2024-05-01 12:00:00,5+02", "2024-05-01t12:00:00z", "2024-05-01T12:00:00.1234567891Z", "2024-05-01T12:00:00+0530", "2024-5-01",
            "9999-12-31T23:59:59Z", "0000-01-01T00:00:00Z", "2262-04-11T23:47:16.854775807Z", "2262-04-11T23:47:16.854775808Z",
            "1677-09-21T00:12:43.145224192Z", "1677-09-21T00:12:43.145224191Z", "2024-05-01T12:00:00Z ", "2024-02-29T23:59:59.999999999-23:59"]
PRICE = ["12.50", "9007199254740993", "-0", "0.25", "1e3", "7", "-2.5", "0", "100", "3.0", "1E2", "0.5"]
PRICE_OTHER = ["12,50", "", " 1", "1 ", "+1", "abc", "0x10", "1e400", "01", "1.", "-", "9223372036854775808", "NaN", "1e"]
ATTR_KEYS = ["color", "size", "n1", "é", "a/b", "~t", "", "k\"q", "shared-prefix-of-a-status-value-0123456789-A"]
WORDS = ["red", "green", "", "blå", "x/y", "t\tab", "z" * 20, "\U0001F600", "ok"]
STYLES = ["none", "spaces", "pretty-lf", "pretty-crlf", "tabs"]
INVALID_KINDS = {
    "trailing comma": "[1,2,]", "missing colon": '{"a" 1}', "missing comma": "[1 2]", "01": "01", "1.": "[1.]", "-": "[-]", "1e400": "1e400",
    "tru": "tru", "\\x": '"a\\xb"', "\\u12G4": '"\\u12G4"',
    # "a code unit in DC00-DFFF on its own is an error" (msj_validate_device, "strings")
    "lone low surrogate": '"\\udc00"',
    # the shallowest nest of arrays that is an error: the innermost opens at depth MAX_DEPTH - 1, its walker depth is MAX_DEPTH
    # ("'[': if it is >= max_depth"); ``Generator.document`` also writes the deepest that is valid
    "depth": "[" * MAX_DEPTH + "1" + "]" * MAX_DEPTH, "second value": '{"a":1 2}'}
# the verdict's code per kind (msj_validate_device: TAPE_ERROR 3, DEPTH_ERROR 4, STRING_ERROR 5, the atom t 6, NUMBER_ERROR 9)
INVALID_CODES = {"trailing comma": 3, "missing colon": 3, "missing comma": 3, "01": 9, "1.": 9, "-": 9, "1e400": 9, "tru": 6, "\\x": 5,
                 "\\u12G4": 5, "lone low surrogate": 5, "depth": 4, "second value": 3}


class Lit:
    """A number (or any scalar) under one spelling"""

    def __init__(self, text):
        self.text = text


class Obj:
    """An object as the pairs written, duplicates included"""

    def __init__(self, pairs):
        self.pairs = list(pairs)


class Frag:
    """Text written verbatim: what makes a document invalid"""

    def __init__(self, text):
        self.text = text


class Escaped:
    """A string written with every character that may be escaped as an escape"""

    def __init__(self, s):
        self.s = s


def summable(text):
    """The number `text` lies on the grid on which msj_aggregate's 'd' sum is the exact sum rounded once"""
    v = json.loads(text)
    f = Fraction(v)
    assert abs(f) < (1 << 64) and (f / SUM_GRID).denominator == 1, text
    return text


class Generator:
    """n documents from one seed: lines [(text, doc | INVALID)], kinds (the invalid kind or None per document), separators
    (what stands behind each document in the stream) and count, how often each feature was drawn"""

    def __init__(self, seed, n):
        self.rng = random.Random(seed)
        self.count = collections.Counter()
        self.kinds = []          # per document: None, or the invalid kind
        self.lines = []          # (text, doc | INVALID)
        self.separators = []     # what stands behind every document
        n_bad = self.rng.randint((7 * n + 99) // 100, 13 * n // 100)
        bad = set(self.rng.sample(range(n), n_bad))
        kinds = list(INVALID_KINDS)
        for k in range(n):
            kind = kinds[(k + seed) % len(kinds)] if k in bad else None
            tree = self.document(k, kind)
            style = self.rng.choice(STYLES)
            self.count["style " + style] += 1
            text = self.emit(tree, style).encode("utf-8")
            self.kinds.append(kind)
            self.lines.append((text, INVALID if kind else value_of(tree)))
        for k in range(n):
            self.separators.append(self.separator(k))

    # ---- the serialiser ----

    def string(self, s, p):
        """The JSON text of s; p: how often a character that may be written either way is escaped"""
        rng, out = self.rng, ['"']
        hexes = lambda u: ("\\u%04x" if rng.random() < 0.5 else "\\u%04X") % u
        for ch in s:
            c = ord(ch)
            if ch in '"\\':
                out.append("\\" + ch)
            elif c < 0x20:
                short = {"\n": "\\n", "\t": "\\t", "\r": "\\r", "\b": "\\b", "\f": "\\f"}.get(ch)
                out.append(short if short and rng.random() < 0.5 else hexes(c))
            elif rng.random() >= p:
                out.append(ch)
            elif ch == "/":
                out.append("\\/")
                self.count["escaped slash"] += 1
            elif c >= 0x10000:
                out.append(hexes(0xD800 + ((c - 0x10000) >> 10)) + hexes(0xDC00 + ((c - 0x10000) & 0x3FF)))
                self.count["surrogate pair"] += 1
            else:
                out.append(hexes(c))
                self.count["escaped non-ascii" if c >= 0x80 else "escaped ascii"] += 1
        return "".join(out) + '"'

    def emit(self, tree, style, level=0):
        colon, comma, nl, indent = {"none": (":", ",", "", ""), "spaces": (": ", ", ", "", ""), "pretty-lf": (": ", ",", "\n", "  "),
                                    "pretty-crlf": (": ", ",", "\r\n", "    "), "tabs": (":\t", ",\t", "", "")}[style]
        if isinstance(tree, (Lit, Frag)):
            return tree.text
        if tree is None or isinstance(tree, bool):
            return {None: "null", True: "true", False: "false"}[tree]
        if isinstance(tree, str):
            return self.string(tree, 0.3)
        if isinstance(tree, Escaped):
            return self.string(tree.s, 1.0)
        pad, inner = nl + indent * level, nl + indent * (level + 1)
        if isinstance(tree, list):
            if not tree:
                return "[]" if self.rng.random() < 0.7 else "[ ]"
            return "[" + inner + (comma + inner).join(self.emit(x, style, level + 1) for x in tree) + pad + "]"
        if not tree.pairs:
            return "{}" if self.rng.random() < 0.7 else "{ }"
        members = []
        for key, value in tree.pairs:
            escaped = self.rng.random() < 0.06 and key != ""
            self.count["escaped key"] += escaped
            members.append(self.string(key, 0.5 if escaped else 0.0) + colon + self.emit(value, style, level + 1))
        return "{" + inner + (comma + inner).join(members) + pad + "}"

    def separator(self, k):
        """Behind document k: a newline, a blank, or -- between a closing and an opening bracket -- nothing"""
        text = self.lines[k][0]
        nxt = self.lines[k + 1][0] if k + 1 < len(self.lines) else b""
        r = self.rng.random()
        if r < 0.15 and text[-1:] in b"}]" and nxt[:1] in (b"{", b"["):
            self.count["separator none"] += 1
            return b""
        if r < 0.3 and k + 1 < len(self.lines):
            self.count["separator blank"] += 1
            return b" "
        return b"\n"

    # ---- the values ----

    def pick(self, feature, choices):
        self.count[feature] += 1
        return self.rng.choice(choices)

    def number(self, pool, feature):
        text = self.rng.choice(pool)
        self.count[feature + " " + text] += 1
        return Lit(text)

    def scalar(self):
        r = self.rng.random()
        if r < 0.35:
            return self.rng.choice(WORDS)
        if r < 0.55:
            return Lit(str(self.rng.randint(-5, 50)))
        if r < 0.7:
            return self.number(UNSUMMED, "unsummed")
        if r < 0.8:
            return Lit(self.rng.choice(LATENCY))
        return self.rng.choice([None, True, False])

    def status(self):
        r = self.rng.random()
        if r < 0.85:
            s = self.rng.choice(STATUS)
            self.count["status " + repr(s)] += 1
            return s
        return self.pick("status no string", [Lit("7"), None, Obj([("code", Lit("1"))]), True, ["active"]])

    def latency(self):
        r = self.rng.random()
        if r < 0.8:
            text = summable(self.rng.choice(LATENCY))
            self.count["latency " + text] += 1
            return Lit(text)
        return self.pick("latency no number", [None, "fast", [Lit("1")], Obj([("ms", Lit("3"))]), "250"])

    def ts(self):
        rng = self.rng
        r = rng.random()
        if r < 0.65:
            y, mo = rng.choice([1970, 1999, 2024, 2024, 2025, 2100]), rng.randint(1, 12)
            d = rng.randint(1, 28)
            if rng.random() < 0.1:
                y, mo, d = 2024, 2, 29
                self.count["ts leap day"] += 1
            s = "%04d-%02d-%02dT%02d:%02d:%02d" % (y, mo, d, rng.randint(0, 23), rng.randint(0, 59), rng.randint(0, 59))
            digits = rng.randint(0, 9)
            if digits:
                s += "." + "".join(rng.choice("0123456789") for _ in range(digits))
            self.count["ts fraction %d" % digits] += 1
            off = rng.choice(["Z", "+", "-"])
            self.count["ts offset " + off] += 1
            s += off if off == "Z" else "%s%02d:%02d" % (off, rng.randint(0, 14), rng.choice([0, 30, 45]))
        elif r < 0.9:
            s = rng.choice(TS_OTHER)
            self.count["ts other"] += 1
        else:
            return self.pick("ts no string", [Lit("1714566896"), None, Lit("1.5")])
        if rng.random() < 0.1:
            self.count["ts escaped"] += 1
            return Escaped(s)
        return s

    def price(self, field):
        rng = self.rng
        r = rng.random()
        if r < 0.6:
            s = summable(rng.choice(PRICE)) if field == "price" else rng.choice(["9007199254740993", "-0", "42"] + [str(rng.randint(0, 10**6))] * 5)
            self.count[field + " number"] += 1
        elif r < 0.85:
            s = rng.choice(PRICE_OTHER) if field == "price" else "k-%d" % rng.randint(0, 99)
            self.count[field + " other"] += 1
        else:
            return self.pick(field + " no string", [Lit(summable("3")), Lit(summable("4.5")), None])
        if rng.random() < 0.1:
            self.count[field + " escaped"] += 1
            return Escaped(s)
        return s

    def tags(self, depth=0):
        rng = self.rng
        r = rng.random()
        if r < 0.15:
            self.count["tags empty"] += 1
            return []
        if r < 0.22:
            return self.pick("tags no list", ["red", None, Obj([("a", Lit("1"))])])
        out = [self.scalar() for _ in range(rng.randint(1, 5))]
        if depth == 0 and rng.random() < 0.15:
            self.count["tags nested"] += 1
            out.insert(rng.randrange(len(out) + 1), [self.scalar() for _ in range(rng.randint(0, 2))])
        return out

    def attrs(self):
        rng = self.rng
        if rng.random() < 0.07:
            return self.pick("attrs no object", ["none", [], None])
        pairs = []
        for _ in range(rng.randint(0, 5)):
            key = rng.choice(ATTR_KEYS)
            self.count["attrs empty key"] += key == ""
            self.count["attrs duplicate key"] += any(key == k for k, _ in pairs)
            pairs.append((key, self.scalar() if rng.random() < 0.8 else Obj([("b", self.scalar())])))
        return Obj(pairs)

    def item(self):
        rng = self.rng
        if rng.random() < 0.05:
            return self.pick("item no object", ["s", Lit("1"), None, []])
        pairs = [("sku", rng.choice(["s0", "s1", "s2", "sé"]) if rng.random() < 0.9 else Lit("5")),
                 ("q", Lit(summable(rng.choice(["0", "1", "2", "-4", "1.5", "0.25", "-0.0", "9007199254740993", "1e2"]))) if rng.random() < 0.85
                  else rng.choice(["2", None])),
                 ("tags", self.tags(1)), ("dims", Obj([("w", self.scalar()), ("h", [Lit(str(rng.randint(0, 4)))])]))]
        rng.shuffle(pairs)
        pairs = [p for p in pairs if rng.random() >= 0.12]
        if pairs and rng.random() < 0.08:
            self.count["item duplicate key"] += 1
            pairs.append((pairs[0][0], self.scalar()))
        return Obj(pairs)

    def items(self):
        if self.rng.random() < 0.06:
            return self.pick("items no list", [None, "none", Obj([])])
        n = self.rng.randint(0, 4)
        self.count["items %d" % n] += 1
        return [self.item() for _ in range(n)]

    def geo(self):
        rng = self.rng
        if rng.random() < 0.1:
            return self.pick("geo scalar", [None, Lit("1e308"), "nowhere", []])
        pairs = [("lat", self.number(UNSUMMED + LATENCY, "geo")), ("lon", [self.scalar() for _ in range(rng.randint(0, 3))])]
        if rng.random() < 0.3:
            pairs.append(("note", Obj([("a\nb", self.scalar()), ("deep", [[Obj([])], []])])))
        return Obj(pairs)

    def document(self, k, kind):
        rng = self.rng
        frag = Frag(INVALID_KINDS[kind]) if kind else None
        if kind:
            self.count["invalid " + kind] += 1
        if kind == "depth" or (kind and rng.random() < 0.15):
            return frag                                    # the root itself
        if not kind and rng.random() < 0.05:
            if rng.random() < 0.2:                         # the deepest array that is valid
                self.count["root deep"] += 1
                return Frag("[" * (MAX_DEPTH - 1) + "1" + "]" * (MAX_DEPTH - 1))
            root = self.pick("root no object", [[Lit("1"), "a", Obj([("status", "active")])], [], Lit("42"), "str", None, True, Lit("-1.5e3"),
                                                Obj([])])
            return root
        makers = [("status", self.status), ("tags", self.tags), ("attrs", self.attrs), ("items", self.items), ("geo", self.geo),
                  ("latency", self.latency), ("ts", self.ts), ("price", lambda: self.price("price")), ("id", lambda: self.price("id"))]
        rng.shuffle(makers)
        pairs = []
        for key, make in makers:
            if rng.random() < 0.1:
                self.count["absent " + key] += 1
                continue
            pairs.append((key, make()))
        for key, make in makers:
            if pairs and rng.random() < 0.04:
                at = rng.randrange(len(pairs) + 1)
                self.count["duplicate before the first" if all(k2 != key for k2, _ in pairs[:at]) and any(k2 == key for k2, _ in pairs[at:])
                           else "duplicate behind the first" if any(k2 == key for k2, _ in pairs[:at]) else "late member"] += 1
                pairs.insert(at, (key, make()))
        if frag is not None:
            at = rng.randrange(len(pairs) + 1)
            pairs.insert(at, (rng.choice(["bad", "status", "geo"]), frag))
        return Obj(pairs)


def value_of(tree):
    """The Python value of a tree the generator wrote: the first of duplicate keys wins"""
    if isinstance(tree, (Lit, Frag)):
        return json.loads(tree.text)
    if isinstance(tree, Escaped):
        return tree.s
    if isinstance(tree, list):
        return [value_of(x) for x in tree]
    if isinstance(tree, Obj):
        out = {}
        for key, value in tree.pairs:
            out.setdefault(key, value_of(value))
        return out
    return tree


_generated = {}


def generate(seed, n):
    if (seed, n) not in _generated:
        _generated[seed, n] = Generator(seed, n)
    return _generated[seed, n]


def lines(seed, n):
    """-> [(text: bytes, doc)]: doc the Python value (the first duplicate wins), or INVALID"""
    return generate(seed, n).lines


def stream(seed, n):
    """The documents with the generator's separators between them -> bytes"""
    g = generate(seed, n)
    return b"".join(t + s for (t, _), s in zip(g.lines, g.separators))


def first_wins(pairs):
    out = {}
    for key, value in pairs:
        out.setdefault(key, value)
    return out


def refuse_constant(name):
    raise ValueError(name)


def python_rejects(text):
    """json.loads refuses the text -- or takes it and gives a string that is no Unicode text (a lone surrogate, which json
    passes through and UTF-8 cannot hold)"""
    try:
        v = json.loads(text, object_pairs_hook=list, parse_constant=refuse_constant)   # (every member kept, duplicates too)
        json.dumps(v, ensure_ascii=False).encode("utf-8")
    except (ValueError, RecursionError):
        return True
    return False


def canon(v):
    """A value with its kind: True is not 1, 1 is not 1.0, and a double is its bit pattern (-0.0 is not 0.0)"""
    if isinstance(v, float):
        return ("d", struct.pack("<d", v))
    if v is None or isinstance(v, (bool, str)):
        return v
    if isinstance(v, int):
        return ("l", v)
    if isinstance(v, (list, tuple)):
        return [canon(x) for x in v]
    return ("o", [(k, canon(x)) for k, x in v.items()])


# ---- what both test files ask ------------------------------------------------------------------------------------------------

SEEDS = [11, 12, 13, 14, 15, 16]
DOCUMENTS = 300
T0 = datetime.datetime(2024, 6, 1, 12, 0, 0, tzinfo=datetime.timezone(datetime.timedelta(hours=2)))
# (specs, cast) of ``where``: each alone, and those without a cast together -- sixteen, the most one call takes
WHERE = [([("/geo/lat", "found")], None), ([("/latency", "type", "number")], None), ([("/tags", "type", ["array", "null", "string"])], None),
         ([("/latency", "==", 9007199254740993)], None), ([("/latency", "==", 9007199254740992.0)], None),
         ([("/latency", "<", 9007199254740993)], None), ([("/latency", "<", 9007199254740994.0)], None),
         ([("/latency", "<=", 0)], None), ([("/latency", "<=", -0.0)], None),
         ([("/latency", ">", 9007199254740992)], None), ([("/latency", ">", 9007199254740992.0)], None),
         ([("/latency", ">=", 9007199254740993)], None), ([("/latency", ">=", 1.5)], None),
         ([("/status", "==", "act\u00edve")], None), ([("/status", "prefix", "shared-prefix-of-a-status-value-0123456789-")], None),
         ([("not", ("/latency", ">", 100))], None),
         ([("/price", ">=", 12.5)], {"/price": "number"}), ([("/ts", ">=", T0)], {"/ts": ("timestamp", "ms")}),
         ([("/price", "<", 100), ("/ts", "<", T0)], {"/price": "number", "/ts": ("timestamp", "s")})]
SELECTION = ([("/latency", "type", "number"), ("/status", "type", "string")], None)    # the ``where`` whose rows stats and order_by run on


def pointers():
    from tests import stream_order as so

    return so.POINTERS + NUMERIC_POINTERS + EXTRA_POINTERS


# ---- the model ------------------------------------------------------------------------------------------------------------

_BLANK = b" \t\n\r"
_NUMBER = re.compile(rb"-?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?")
_TIMESTAMP = re.compile(rb"([0-9]{4})-([0-9]{2})-([0-9]{2})(?:[Tt ]([0-9]{2}):([0-9]{2})(?::([0-9]{2})(?:[.,]([0-9]{1,9}))?)?"
                        rb"(?:([Zz])|([+-])([0-9]{2})(?::?([0-9]{2}))?)?)?")
_EPOCH = datetime.datetime(1970, 1, 1, tzinfo=datetime.timezone.utc)
PER_SECOND = {"s": 1, "ms": 10**3, "us": 10**6, "ns": 10**9}
TYPE_TAGS = {"object": "{", "array": "[", "string": '"', "int": "l", "double": "d", "number": "ld", "true": "t", "false": "f", "bool": "tf",
             "null": "n"}


def _blanks(t, i):
    while i < len(t) and t[i] in _BLANK:
        i += 1
    return i


def _end(t, i):
    """The index behind the value that starts at t[i]"""
    if t[i] == 0x22:
        i += 1
        while t[i] != 0x22:
            i += 2 if t[i] == 0x5C else 1
        return i + 1
    if t[i] in b"{[":
        depth = 0
        while True:
            if t[i] == 0x22:
                i = _end(t, i)
                continue
            depth += (t[i] in b"{[") - (t[i] in b"}]")
            i += 1
            if depth == 0:
                return i
    while i < len(t) and t[i] not in b" \t\n\r,:]}":
        i += 1
    return i


class Node:
    """A value where it stands in its document's text: t[a:b]"""
    __slots__ = ("t", "a", "b", "kids", "first")

    def __init__(self, t, a, b):
        self.t, self.a, self.b, self.kids, self.first = t, a, b, None, None

    @property
    def text(self):
        return self.t[self.a:self.b]

    @property
    def tag(self):
        """The tape's tag: an integer literal -- no fraction, no exponent -- is an 'l' (msj_number_values_device, "integer")"""
        c = chr(self.t[self.a])
        if c in '{["tfn':
            return c
        return "d" if any(x in self.text for x in (b".", b"e", b"E")) else "l"

    def value(self):
        return json.loads(self.text.decode("utf-8"), object_pairs_hook=first_wins)

    def children(self):
        """The element nodes of an array, or the (key node, value node) pairs of an object, in document order"""
        if self.kids is not None:
            return self.kids                                # (found once: the text does not change)
        t, i, out = self.t, _blanks(self.t, self.a + 1), []
        pairs = t[self.a] == 0x7B
        while t[i] not in b"}]":
            key = None
            if pairs:
                key = Node(t, i, _end(t, i))
                i = _blanks(t, _blanks(t, key.b) + 1)      # (behind the colon)
            value = Node(t, i, _end(t, i))
            out.append((key, value) if pairs else value)
            i = _blanks(t, value.b)
            if t[i] == 0x2C:
                i = _blanks(t, i + 1)
        self.kids = out
        return out

    def get(self, key):
        """The member `key` of an object: the first duplicate wins (msj_select_documents_device, "the SMALLEST such i")"""
        if self.first is None:
            self.first = {}
            for k, v in self.children():
                self.first.setdefault(k.value(), v)
        return self.first.get(key)


def segments(pointer):
    return [s.replace("~1", "/").replace("~0", "~") for s in pointer.split("/")[1:]]


def number_value(node):
    """The number a record carries: an int for an 'l', a float for a 'd', None for anything else"""
    return node.value() if node is not None and node.tag in "ld" else None


def string_value(node):
    """The unescaped UTF-8 of a string value, None for anything else"""
    return node.value().encode("utf-8") if node is not None and node.tag == '"' else None


def compact(text):
    """The text with the blanks outside strings removed"""
    out, i = bytearray(), 0
    while i < len(text):
        if text[i] == 0x22:
            j = _end(text, i)
            out += text[i:j]
            i = j
            continue
        if text[i] not in _BLANK:
            out.append(text[i])
        i += 1
    return bytes(out)


def cast_number(value):
    """msj_cast_strings_device, MSJ_CAST_NUMBER: the bytes `value`, whole, as one JSON number -> int, float or None"""
    if len(value) > 128 or not _NUMBER.fullmatch(value):
        return None
    if any(c in value for c in b".eE"):
        v = float(value)
        return None if v in (float("inf"), float("-inf")) else v
    v = int(value)
    return v if INT64_MIN <= v <= INT64_MAX else None


def cast_timestamp(value, unit):
    """msj_cast_strings_device, MSJ_CAST_TIMESTAMP -> the int64 count of `unit` since 1970-01-01T00:00:00Z, or None"""
    m = _TIMESTAMP.fullmatch(value) if len(value) <= 35 else None
    if not m:
        return None
    y, mo, d, hh, mm, ss, frac, z, sign, oh, om = m.groups()
    y, mo, d, hh, mm, ss = (int(x or 0) for x in (y, mo, d, hh, mm, ss))
    try:
        # (datetime has no year 0: the proleptic Gregorian calendar repeats every 400 years, 146 097 days)
        days = datetime.date(y + 400 if y == 0 else y, mo, d).toordinal() - datetime.date(1970, 1, 1).toordinal() - (146097 if y == 0 else 0)
    except ValueError:
        return None
    if hh > 23 or mm > 59 or ss > 59 or int(oh or 0) > 23 or int(om or 0) > 59:
        return None
    offset = (int(oh or 0) * 3600 + int(om or 0) * 60) * (-1 if sign == b"-" else 1)
    per = PER_SECOND[unit]
    digits = (frac or b"").ljust(9, b"0")
    v = (days * 86400 + hh * 3600 + mm * 60 + ss - offset) * per + int(digits) // (10**9 // per)
    return v if INT64_MIN <= v <= INT64_MAX else None


def datetime_units(when, unit):
    """A datetime operand of ``where`` in the column's unit (``Window.where``: naive means UTC; a floor)"""
    if when.tzinfo is None:
        when = when.replace(tzinfo=datetime.timezone.utc)
    micros = (when - _EPOCH) // datetime.timedelta(microseconds=1)
    per = PER_SECOND[unit]
    return micros * (per // 10**6) if per >= 10**6 else micros // (10**6 // per)


def cast(nodes, spec, keep_numbers=None):
    """msj_cast_strings_device over a column's nodes: per row the number (int / float) or None.  keep_numbers None: what
    ``where`` / ``stats`` / ``order`` ask for -- "number" keeps a value that already is a number, a timestamp does not
    (``_cast_for_filter``, ``_stats``, ``_order``)"""
    kind, unit = (spec, "ns") if isinstance(spec, str) else spec
    keep_numbers = kind == "number" if keep_numbers is None else keep_numbers
    out = []
    for node in nodes:
        s = string_value(node)
        if s is not None:
            out.append(cast_number(s) if kind == "number" else cast_timestamp(s, unit))
        else:
            out.append(number_value(node) if keep_numbers else None)
    return out


def aggregate(values):
    """msj_aggregate of one group's rows: values int / float / None per row -> what ``GroupStats.to_python`` gives"""
    have = [v for v in values if v is not None]
    out = {"n_rows": len(values), "n_values": len(have), "sum": None, "min": None, "max": None, "flags": 0}
    if not have:
        return out
    if all(isinstance(v, int) for v in have):
        total = sum(have)
        if INT64_MIN <= total <= INT64_MAX:
            out["sum"] = total
        else:
            out["sum"], out["flags"] = float(total), 1           # MSJ_AGG_INT_OVERFLOW; int -> float rounds once, ties to even
    else:
        total = sum(Fraction(v) for v in have)
        out["sum"] = total.numerator / total.denominator if total else 0.0   # (int / int is correctly rounded)
    for name, pick, zero in (("min", min, -0.0), ("max", max, 0.0)):
        best = pick(Fraction(v) for v in have)
        equal = [v for v in have if Fraction(v) == best]
        ints = [v for v in equal if isinstance(v, int)]
        if ints:
            out[name] = ints[0]                                   # "Between equal reals the 'l' record wins"
        elif best == 0 and any(struct.pack("<d", v) == struct.pack("<d", zero) for v in equal):
            out[name] = zero                                      # "among doubles -0.0 lies below +0.0"
        else:
            out[name] = equal[0]
    return out


def order(values, rows=None, descending=False, limit=None, values_only=False):
    """msj_sort_rows_device: the entries of `rows` (default: every row) by values[row] as real numbers, stable, rows
    without a value last (or left out)"""
    rows = list(range(len(values))) if rows is None else list(rows)
    have = [k for k in rows if values[k] is not None]
    have.sort(key=lambda k: Fraction(values[k]), reverse=descending)      # (stable in both directions)
    out = have + ([] if values_only else [k for k in rows if values[k] is None])
    return out if limit is None else out[:limit]


def string_ranks(strings):
    """The cast "string" of ``order``: per row the rank of its bytes among the distinct values, None without a string"""
    distinct = sorted(set(s for s in strings if s is not None))
    return [None if s is None else distinct.index(s) for s in strings]


def dictionary(strings, prior=()):
    """msj_dictionary_device / _extend_: (codes, values, first): codes in the order of first appearance behind `prior`"""
    values, first, codes = list(prior), [-1] * len(prior), []
    for k, s in enumerate(strings):
        if s is None:
            codes.append(-1)
            continue
        if s not in values:
            values.append(s)
            first.append(k)
        codes.append(values.index(s))
    return codes, values, first


def join(left, right, how):
    """msj_join_rows_device over byte keys (None: no key) -> [(l, r | None)] in ascending l and, inside a row, ascending r"""
    out = []
    for l, key in enumerate(left):
        match = [r for r, other in enumerate(right) if key is not None and other == key]
        if how == "inner":
            out += [(l, r) for r in match]
        elif how == "left":
            out += [(l, r) for r in match] or [(l, None)]
        elif how == "semi":
            out += [(l, match[0])] if match else []
        else:
            out += [] if match else [(l, None)]
    return out


def array_too_deep(v, depth, max_depth):
    """msj_validate_device, "depth": a non-empty container opened at depth d has walker depth d + 1; '{' is an error when
    that is > max_depth, '[' when it is >= max_depth"""
    if isinstance(v, dict) and v:
        return depth + 1 > max_depth or any(array_too_deep(x, depth + 1, max_depth) for x in v.values())
    if isinstance(v, list) and v:
        return depth + 1 >= max_depth or any(array_too_deep(x, depth + 1, max_depth) for x in v)
    return False


_roots = {}


def root_of(t):
    """The root value's node of a document's text, kept: what a node has found of its children stays found"""
    if t not in _roots:
        _roots[t] = Node(t, _blanks(t, 0), _end(t, _blanks(t, 0)))
    return _roots[t]


class Model:
    """What every view of a window over `lines` ([(text, doc | INVALID)]) returns.  A row is a ``Node`` or None: a document
    with a verdict code, a missing key or a lookup through something that is no object has no value."""

    def __init__(self, lines):
        self.lines = list(lines)
        self.roots = [None if doc is INVALID else root_of(t) for t, doc in self.lines]
        self.invalid = [k for k, r in enumerate(self.roots) if r is None]
        self.columns = {}

    def __len__(self):
        return len(self.roots)

    def at(self, pointer, rows=None):
        """The nodes of a pointer's column: one per row of `rows` (default: the documents)"""
        if rows is None and pointer in self.columns:
            return self.columns[pointer]
        out = []
        for node in (self.roots if rows is None else rows):
            for key in segments(pointer):
                node = node.get(key) if node is not None and node.tag == "{" else None
            out.append(node)
        if rows is None:
            self.columns[pointer] = out
        return out

    # every view below takes the column's nodes

    @staticmethod
    def values(nodes):
        return [None if n is None else canon(n.value()) for n in nodes]

    @staticmethod
    def number_column(nodes, kind):
        """kind "l": (the int64, valid) ; "d": (the double's bytes, valid); 0 where not valid"""
        if kind == "l":
            return [(n.value(), True) if n is not None and n.tag == "l" else (0, False) for n in nodes]
        return Model.doubles([number_value(n) for n in nodes])

    @staticmethod
    def doubles(numbers):
        return [(struct.pack("<d", float(v)), True) if v is not None else (struct.pack("<d", 0.0), False) for v in numbers]

    @staticmethod
    def ints(numbers):
        return [(v, True) if isinstance(v, int) else (0, False) for v in numbers]

    @staticmethod
    def strings(nodes):
        return [string_value(n) for n in nodes]

    @staticmethod
    def raw(nodes, compacted=False):
        return [None if n is None else compact(n.text) if compacted else n.text for n in nodes]

    @staticmethod
    def elements(nodes):
        """Per row the element nodes of an array, None where the row is no array"""
        return [n.children() if n is not None and n.tag == "[" else None for n in nodes]

    @staticmethod
    def entries(nodes):
        """Per row the (key node, value node) pairs of an object, duplicates kept, None where the row is no object"""
        return [n.children() if n is not None and n.tag == "{" else None for n in nodes]

    @staticmethod
    def schema(entries):
        """``MapColumn.schema``: (key, entries, tags) per distinct key in the order of first appearance"""
        seen = {}
        for row in entries:
            for k, v in row or []:
                count, tags = seen.setdefault(k.value(), [0, set()])
                seen[k.value()][0] = count + 1
                tags.add(v.tag)
        return [(key, count, tags) for key, (count, tags) in seen.items()]

    def predicate(self, spec, rows, casts):
        """One spec of ``where`` over `rows` -> [bool]"""
        if len(spec) == 2 and spec[0] == "not":
            return [not x for x in self.predicate(spec[1], rows, casts)]
        pointer, op = spec[0], spec[1]
        nodes = self.at(pointer, rows)
        if pointer in casts:
            numbers = cast(nodes, casts[pointer])
            tags = [None if v is None else "l" if isinstance(v, int) else "d" for v in numbers]
            strs = [None] * len(nodes)
        else:
            numbers, tags, strs = [number_value(n) for n in nodes], [n.tag if n is not None else None for n in nodes], self.strings(nodes)
        if op == "found":
            return [t is not None for t in tags]
        operand = spec[2]
        if op == "type":
            names = [operand] if isinstance(operand, str) else operand
            return [t is not None and any(t in TYPE_TAGS[name] for name in names) for t in tags]
        if isinstance(operand, datetime.datetime):
            operand = datetime_units(operand, casts[pointer][1])
        if isinstance(operand, (str, bytes)):
            operand = operand.encode("utf-8") if isinstance(operand, str) else operand
            return [s is not None and (s == operand if op == "==" else s.startswith(operand)) for s in strs]
        compare = {"==": lambda x: x == operand, "<": lambda x: x < operand, "<=": lambda x: x <= operand, ">": lambda x: x > operand,
                   ">=": lambda x: x >= operand}[op]      # (Python compares an int with a float exactly)
        return [v is not None and compare(v) for v in numbers]

    def where(self, specs, any_=False, cast=None, rows=None):
        """The numbers of the rows that ``where`` keeps"""
        rows = self.roots if rows is None else rows
        said = [self.predicate(s, rows, cast or {}) for s in specs]
        return [k for k in range(len(rows)) if (any if any_ else all)(column[k] for column in said)]

    def stats(self, columns, keys=None, n_groups=None):
        """``GroupStats.to_python`` of `columns` {name: [int | float | None] per row}; keys: (codes, values) or None"""
        names = list(columns)
        rows = len(columns[names[0]])
        if keys is None:
            groups, labels = [list(range(rows))], [None]
        else:
            codes, values = keys
            G = len(values) if n_groups is None else n_groups
            groups, labels = [[k for k in range(rows) if codes[k] == g] for g in range(G)], values
        out = []
        for g, members in enumerate(groups):
            row = {} if keys is None or labels is None else {"key": labels[g].decode("utf-8")}
            for name in names:
                row[name] = aggregate([columns[name][k] for k in members])
            out.append(row)
        return out
