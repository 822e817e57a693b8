"""Reader of include/sfh_amd.h: the C ABI as ctypes, so that Python states it nowhere a second time.

It understands the dialect the header is written in and nothing more - after comments are stripped: ``#define SFH_X <integer>``
or ``(<negative integer>)``, ``typedef struct sfh_x { type a, b[3], c[4][64]; ... } sfh_x;`` and prototypes
``ret sfh_name(type name, ...);``.  Anything else raises ``SfhError`` with the header line; there is no partial result.
"""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sfh_amd.h")

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "long long": C.c_longlong, "uint32_t": C.c_uint32,
           "uint16_t": C.c_uint16, "uint8_t": C.c_uint8, "float": C.c_float, "double": C.c_double}
POINTEES = ("void", "char", "int8_t", "uint64_t")     # type words that only ever stand behind a pointer

_CPLUSPLUS = re.compile(r"^[ \t]*#ifdef\b.*?^[ \t]*#endif\b.*?$", re.M | re.S)      # each holds one brace of `extern "C" { }`
_DIRECTIVE = re.compile(r"^[ \t]*(#\w*)[ \t]*(\w*)[ \t]*(.*?)[ \t]*$", re.M)
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;")
_PROTO = re.compile(r"([\w\s*]+?[\s*])(\w+)\s*\(([^(){};]*)\)\s*;")
_DECLARATOR = r"\w+(?:\[\d+\])*"
_MEMBER = re.compile(r"\s*([^;]+?[\s*])(%s(?:\s*,\s*%s)*)\s*;" % (_DECLARATOR, _DECLARATOR), re.S)
_PARAM = re.compile(r"\s*(.+?[\s*])\w+\s*", re.S)
_SPACE = re.compile(r"\s*")


class SfhError(RuntimeError):
    pass


def _line_ends(m):
    return " " + "\n" * m.group().count("\n")


class Abi:
    """``defines``: name -> int.  ``structs``: name -> ctypes.Structure, members in the header's order.  ``functions``:
    name -> (return type, [parameter types]) as C text, e.g. ``"const uint8_t* const*"``; ``signatures()`` gives them as ctypes."""

    def __init__(self, text, origin="sfh_amd.h"):
        self.defines, self.structs, self.functions = {}, {}, {}
        self._origin, self._known = origin, {}
        # whatever is cut out leaves its line ends behind: an offset into `_body` always lies on its line of the file
        body = re.sub(r"/\*.*?\*/", _line_ends, text, flags=re.S)
        body = self._body = _CPLUSPLUS.sub(_line_ends, body)
        for m in _DIRECTIVE.finditer(body):
            word, name, value = m.groups()
            if word == "#define" and value:       # a define without a value is the include guard
                if not re.fullmatch(r"\d+|\(-\d+\)", value):
                    self._fail(m.start(), f"#define {name}: {value!r} is not an integer literal")
                self.defines[name] = int(value.strip("()"))
            elif word not in ("#define", "#ifndef", "#include", "#endif"):
                self._fail(m.start(), f"preprocessor line {m.group().strip()!r}")
        body = self._body = _DIRECTIVE.sub("", body)
        pos = _SPACE.match(body).end()
        while pos < len(body):
            m = _STRUCT.match(body, pos)
            if m:
                self._struct(m.group(1), m.group(2), m.start(2))
            else:
                m = _PROTO.match(body, pos)
                if not m:
                    self._fail(pos, f"cannot segment the declaration starting {body[pos:pos + 60].splitlines()[0]!r}")
                params = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
                self.functions[m.group(2)] = (self._canon(m.group(1), pos), [self._param(p, pos) for p in params])
            pos = _SPACE.match(body, m.end()).end()

    def _fail(self, pos, what):
        raise SfhError(f"{self._origin}:{self._body.count(chr(10), 0, pos) + 1}: {what}")

    def ctype(self, text, pos=0, ret=False):
        """the ctypes type of a C type: the scalar table, a structure declared earlier, ``c_void_p`` for every pointer
        (``c_char_p`` for a returned ``const char*``)"""
        words = re.findall(r"\w+|\*", text)
        base = " ".join(w for w in words if w not in ("const", "*"))
        if base not in SCALARS and base not in self.structs and not ("*" in words and base in POINTEES):
            self._fail(pos, f"unknown type {base!r} in {' '.join(text.split())!r}")
        if "*" in words:
            return C.c_char_p if ret and base == "char" else C.c_void_p
        return SCALARS.get(base) or self.structs[base]

    def _canon(self, text, pos):
        """a type as segmented -> one spelling, e.g. ``const uint8_t* const*``; raises for a type outside the vocabulary"""
        if text not in self._known:
            self.ctype(text, pos)
            self._known[text] = re.sub(r"\s*\*", "*", " ".join(text.split()))
        return self._known[text]

    def _param(self, text, pos):
        m = _PARAM.fullmatch(text)
        if not m:
            self._fail(pos, f"cannot segment the parameter {' '.join(text.split())!r}")
        return self._canon(m.group(1), pos)

    def _struct(self, name, body, pos):
        fields, at = [], _SPACE.match(body).end()
        while at < len(body):
            m = _MEMBER.match(body, at)
            if not m:
                self._fail(pos + at, f"struct {name}: cannot segment the member starting {body[at:at + 60].splitlines()[0]!r}")
            for d in m.group(2).split(","):
                typ = self.ctype(m.group(1), pos + at)
                for n in reversed(re.findall(r"\[(\d+)\]", d)):
                    typ = typ * int(n)
                fields.append((d.split("[")[0].strip(), typ))
            at = _SPACE.match(body, m.end()).end()
        self.structs[name] = type(name, (C.Structure,), {"_fields_": fields, "__doc__": f"struct {name} of include/sfh_amd.h"})

    def signatures(self, typed=()):
        """name -> (restype, [argtypes]); ``typed``: C type text -> ctypes type for the few pointers that are not bound as
        ``c_void_p``"""
        typed = dict(typed)
        return {n: (self.ctype(r, ret=True), [typed.get(a) or self.ctype(a) for a in args]) for n, (r, args) in self.functions.items()}


def read(path=HEADER):
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise SfhError(f"{path}: the C ABI header cannot be read ({e.strerror}); the binding is derived from it") from None
    return Abi(text, os.path.basename(path))
