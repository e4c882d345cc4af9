"""The one reader of include/fhestring_hip.h: every function, constant and struct of the C ABI as C-level descriptions.

The ctypes binding (_lib.py), the Python constants (api.py, parallel.py) and the Rust binding
(tools/gen_rust_bindings.py) are all derived from what parse_header() returns; none of them describes the header again.
"""
import collections
import functools
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fhestring_hip.h")

SCALARS = ("int", "size_t", "uint64_t", "uint32_t", "uint8_t", "int64_t", "int32_t", "double", "char", "void")

# `const uint64_t *` -> CType("uint64_t", True, 1).  const is the pointee's; `T **` is an out-parameter that receives a
# pointer; an array parameter (`uint32_t key[8]`) has decayed to ptr = 1.
CType = collections.namedtuple("CType", "base const ptr")


def _need(ok, what):
    if not ok:
        raise ValueError("cannot parse %r" % (what,))


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def parse_type(words, stars, known):
    base = [w for w in words if w not in ("const", "struct")]
    _need(len(base) == 1 and (base[0] in SCALARS or base[0] in known), words)      # one known type name
    _need(stars or base[0] != "void", words)
    return CType(base[0], "const" in words, stars)


def parse_param(p, known):
    p = re.sub(r"\*\s*const\s*\*", "**", p.strip())          # `const T *const *x`: an array of pointers that is only read
    m = re.match(r"^(.*?)(\**)\s*([A-Za-z_]\w*)\s*((?:\[[^\]]*\])*)$", p.replace(" *", "*").replace("* ", "*"))
    _need(m, p)
    stars = len(m.group(2)) + (1 if m.group(4) else 0)       # `uint32_t key[8]` decays to a pointer
    return m.group(3), parse_type(m.group(1).split(), stars, known)


def _parse(text):
    text = strip_comments(text)
    out = {"consts": [], "opaque": [], "aliases": [], "fnptrs": [], "structs": [], "funcs": []}
    env = {}
    for m in re.finditer(r"^#define\s+(FHS_\w+)\s+(.+)$", text, flags=re.M):
        expr = re.sub(r"\(\s*size_t\s*\)", "", m.group(2)).strip()
        _need(re.fullmatch(r"[\w\s()*+\-]+", expr), expr)
        val = eval(expr, {"__builtins__": {}}, dict(env))     # integer arithmetic over earlier FHS_ constants only
        env[m.group(1)] = val
        out["consts"].append((m.group(1), val))
    body = re.sub(r"^#.*$", "", text, flags=re.M)
    body = body.replace('extern "C" {', "")
    known = set()
    # struct typedefs with fields first (their names are types of later declarations)
    for m in re.finditer(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", body, flags=re.S):
        fields = []
        for decl in m.group(1).split(";"):
            decl = decl.strip()
            if not decl:
                continue
            ty, names = decl.split(None, 1)
            for n in names.split(","):
                fields.append((n.strip(), parse_type([ty], 0, known)))
        out["structs"].append((m.group(2), fields))
        known.add(m.group(2))
    body = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", "", body, flags=re.S)
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s+(\w+)\s*;", body):
        out["opaque"].append(m.group(2))
        known.add(m.group(2))
    for m in re.finditer(r"typedef\s+(\w+)\s+(\w+)\s*;", body):
        out["aliases"].append((m.group(2), parse_type([m.group(1)], 0, known)))
        known.add(m.group(2))
    for m in re.finditer(r"typedef\s+(\w+)\s*\(\s*\*\s*(\w+)\s*\)\s*\((.*?)\)\s*;", body, flags=re.S):
        args = [parse_param(p, known) for p in m.group(3).split(",")]
        out["fnptrs"].append((m.group(2), parse_type([m.group(1)], 0, known), args))
        known.add(m.group(2))
    body = re.sub(r"typedef[^;]*;", "", body)
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt or stmt == "}":
            continue
        m = re.match(r"^(.*?)(\**)\s*(fhs_\w+)\s*\((.*)\)$", stmt.replace(" *", "*"))
        _need(m, stmt)
        ret_words, ret_stars = m.group(1).split(), len(m.group(2))
        ret = None if (ret_words == ["void"] and ret_stars == 0) else parse_type(ret_words, ret_stars, known)
        params = m.group(4).strip()
        args = [] if params == "void" else [parse_param(p, known) for p in params.split(",")]
        out["funcs"].append((m.group(3), ret, args))
    return out


@functools.lru_cache(maxsize=None)
def parse_header(path=HEADER):
    """-> dict(consts=[(name, int)], opaque=[name], aliases=[(name, CType)], fnptrs=[(name, ret, [(arg, CType)])],
    structs=[(name, [(field, CType)])], funcs=[(name, ret CType or None, [(arg, CType)])]) in header order.  Read once
    per process; a missing or unparsable header is an FhsError."""
    from ._lib import FhsError
    try:
        with open(path) as f:
            return _parse(f.read())
    except (OSError, ValueError, NameError, SyntaxError) as e:
        raise FhsError("cannot read the C ABI from %s: %s: %s" % (path, type(e).__name__, e))
