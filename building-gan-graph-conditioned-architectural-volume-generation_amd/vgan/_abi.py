"""Reader of the C ABI header (``include/vgan.h``): its integer ``#define``s,
one ``ctypes.Structure`` per ``typedef struct`` and ``(restype, argtypes)`` per
prototype, so that the header is the binding's only source.

It reads exactly the dialect the header is written in -- ``typedef struct [tag]
{ ... } name;`` blocks, fixed-width scalars, pointers, arrays sized by a
literal or a ``#define``, comma-declared fields (``int32_t lda, ldb;``) and
plain prototypes -- and raises ``ImportError`` naming the header line for
anything else: a wrong guess here would corrupt the arguments of a native call.
"""
from __future__ import annotations

import ctypes
import keyword
import os
import re
from typing import NamedTuple

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double,
            **{f"{u}int{b}_t": getattr(ctypes, f"c_{u}int{b}") for u in ("", "u") for b in (8, 16, 32, 64)}}
_POINTEES = ("void", "char")  # types only behind a '*'

# "[const] T [* [const]]... [name] [[bound]]"
_DECL = re.compile(r"\s*(?:const\s+)?(\w+)((?:\s*\*\s*(?:const\b\s*)?)*)\s*(\w*)\s*(?:\[\s*(\w+)\s*\])?\s*")
_STATEMENT = re.compile(r"\s*((?:[^;{}]|\{[^{}]*\})+);")
_STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{(.*)\}\s*(\w+)\s*", re.S)
_PROTOTYPE = re.compile(r"(.*?)\b(\w+)\s*\(([^()]*)\)\s*", re.S)


class Abi(NamedTuple):
    constants: dict   # NAME -> int, every integer #define
    structs: dict     # C name -> ctypes.Structure subclass, in header order
    signatures: dict  # function -> (restype, [argtypes]), every prototype


def camel(c_name: str) -> str:
    """vg_gen_ln_layer -> VgGenLnLayer: the mirror's class name."""
    return "".join(p.capitalize() for p in c_name.split("_"))


def _blank(m) -> str:
    return re.sub(r"[^\n]", " ", m.group())  # keeps every offset and line number


def parse(text: str, where: str = "vgan.h") -> Abi:
    constants, structs, signatures = {}, {}, {}

    def fail(pos: int, why: str):
        raise ImportError(f"{where}:{text.count(chr(10), 0, pos) + 1}: {why}")

    def decl(src: str, pos: int, returned: bool = False):
        m = _DECL.fullmatch(src)
        if not m:
            fail(pos, f"cannot read the declaration {' '.join(src.split())!r}")
        base, stars, name, bound = m.group(1), m.group(2).count("*"), m.group(3), m.group(4)
        if (base not in _SCALARS and base not in structs and not (stars and base in _POINTEES)
                and not (returned and base == "void")):
            fail(pos, f"unknown type {base!r}")
        return base, stars, name, bound

    text = re.sub(r"/\*.*?\*/|//[^\n]*", _blank, text, flags=re.S)
    for m in re.finditer(r"^[ \t]*#[ \t]*(\w+)[ \t]*([^\n]*)$", text, flags=re.M):
        kind, rest = m.group(1), m.group(2).split(None, 1)
        if kind == "define" and len(rest) == 2:
            value = re.fullmatch(r"\(?\s*(-?\d+)\s*\)?", rest[1].strip())
            if not value:
                fail(m.start(), f"#define {rest[0]} is not an integer literal")
            constants[rest[0]] = int(value.group(1))
        elif kind not in ("define", "include", "ifndef", "endif") and (kind, rest) != ("ifdef", ["__cplusplus"]):
            fail(m.start(), f"unsupported directive #{kind} {m.group(2)}".rstrip())
    text = re.sub(r"^[ \t]*#[^\n]*$", _blank, text, flags=re.M)
    text, n = re.subn(r'extern\s+"C"\s*\{', _blank, text)
    if n:  # ... and its closing brace, the header's last
        close = text.rindex("}")
        text = text[:close] + " " + text[close + 1:]

    def new(name: str, pos: int):
        if name in structs or name in signatures:
            fail(pos, f"{name} is declared twice")

    def struct(body: str, pos: int, name: str):
        new(name, pos)
        fields = []
        for f in re.finditer(r"[^;]+;|\S[^;]*$", body):
            at = pos + f.end() - len(f.group().lstrip())
            if not f.group().endswith(";"):
                fail(at, "a field without its ';'")
            first, *more = f.group()[:-1].split(",")
            if not first.strip():
                continue
            base = decl(first, at)[0]
            for d in [first] + [f"{base} {d}" for d in more]:
                base, stars, field, bound = decl(d, at)
                if not field:
                    fail(at, "a field without a name")
                t = ctypes.c_void_p if stars else structs.get(base) or _SCALARS[base]
                if bound is not None:
                    if not bound.isdigit() and bound not in constants:
                        fail(at, f"array bound {bound!r} is neither a literal nor a known #define")
                    t = t * (int(bound) if bound.isdigit() else constants[bound])
                fields.append((field + "_" if keyword.iskeyword(field) else field, t))
        structs[name] = type(camel(name), (ctypes.Structure,),
                             {"_fields_": fields, "__doc__": f"{name} ({os.path.basename(where)})"})

    def prototype(ret: str, pos: int, name: str, params: str):
        new(name, pos)
        base, stars, extra, bound = decl(ret, pos, returned=True)
        if extra or bound:
            fail(pos, f"cannot read the return type {' '.join(ret.split())!r}")
        if stars:
            res = ctypes.c_char_p if base == "char" else ctypes.c_void_p
        elif base in structs:
            fail(pos, "a struct returned by value")
        else:
            res = _SCALARS[base] if base != "void" else None
        args = []
        for p in [] if params.strip() in ("", "void") else params.split(","):
            base, stars, _, bound = decl(p, pos)
            if bound is not None or (not stars and base in structs):
                fail(pos, f"parameter {' '.join(p.split())!r}: an array or a struct by value")
            # a pointer to a header struct takes byref(mirror), an array of mirrors or None -- and no other struct
            args.append(_SCALARS[base] if not stars else
                        ctypes.POINTER(structs[base]) if stars == 1 and base in structs else ctypes.c_void_p)
        signatures[name] = (res, args)

    pos = 0
    while m := _STATEMENT.match(text, pos):
        at, s = m.start(1), m.group(1)
        if t := _STRUCT.fullmatch(s):
            struct(t.group(1), at + t.start(1), t.group(2))
        elif t := _PROTOTYPE.fullmatch(s):
            prototype(t.group(1), at, t.group(2), t.group(3))
        else:
            fail(at, "neither a typedef struct nor a prototype")
        pos = m.end()
    if text[pos:].strip():
        fail(pos + len(text[pos:]) - len(text[pos:].lstrip()), "cannot read this declaration")
    return Abi(constants, structs, signatures)


def read(path: str) -> Abi:
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise ImportError(f"{path}: the C ABI header is required to bind libvgan_hip.so ({e})") from e
    return parse(text, path)
