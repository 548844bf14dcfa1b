"""How the C entry points open (csrc/common.hpp: entry, ctx_entry, host_entry).

1. Every function the headers declare as `polee_status polee_*(<context or handle> *, ...)` is called in one child process with
   every pointer null and every number zero: it returns POLEE_ERR_BAD_ARG and names itself in polee_last_error(NULL).  No GPU is
   touched on that path.  The argument kinds come from the declared parameter types (float and double are passed by value).
2. Every definition of a status-returning `polee_*` function under csrc has one of the three openers as its first statement."""
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADERS = [os.path.join(ROOT, "include", h) for h in ("polee_hip.h", "polee_hip_debug.h")]
CSRC = os.path.join(ROOT, "polee_amd", "csrc")
POLEE_ERR_BAD_ARG = 1

# functions left out of the null-argument scan, each with its reason (at most five)
EXEMPT = {}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _headers_text():
    return "\n".join(_strip_comments(open(h).read()) for h in HEADERS)


def _kind(param):
    """ctypes kind of one declared parameter"""
    p = param.strip()
    if "*" in p or "[" in p or re.search(r"\b\w+_fn\b", p):
        return "ptr"
    words = [w for w in re.findall(r"\w+", p) if w != "const"]
    typ = words[0] if len(words) > 1 else p  # (the last word is the parameter's name)
    if typ == "unsigned" and len(words) > 2:
        typ = words[1]
    kinds = {"float": "f32", "double": "f64", "int": "i32", "unsigned": "i32", "int32_t": "i32", "uint32_t": "i32", "int64_t": "i64",
             "uint64_t": "i64", "size_t": "i64", "long": "i64"}
    assert typ in kinds, "a parameter type this test does not know: %r" % p
    return kinds[typ]


def declared_entry_points():
    """[(name, [kind, ...])] of the declared status functions whose first parameter is a context or a handle"""
    text = _headers_text()
    handles = set(re.findall(r"typedef\s+struct\s+(polee_\w+)\s+\1\s*;", text))
    assert "polee_ctx" in handles and "polee_vi" in handles
    out = []
    for name, params in re.findall(r"\bpolee_status\s+(polee_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        parts = [q for q in params.split(",") if q.strip() and q.strip() != "void"]
        m = re.match(r"\s*(?:const\s+)?(polee_\w+)\s*\*\s*\w+\s*$", parts[0]) if parts else None
        if m and m.group(1) in handles:
            out.append((name, [_kind(q) for q in parts]))
    return out


CHILD = r"""
import ctypes as C, json, sys
lib = C.CDLL(sys.argv[1])
lib.polee_last_error.restype = C.c_char_p
lib.polee_last_error.argtypes = [C.c_void_p]
kinds = {"ptr": (C.c_void_p, None), "f32": (C.c_float, 0.0), "f64": (C.c_double, 0.0), "i32": (C.c_int32, 0), "i64": (C.c_int64, 0)}
for name, params in json.loads(sys.argv[2]):
    print("CALL", name, flush=True)
    f = getattr(lib, name)
    f.restype = C.c_int
    f.argtypes = [kinds[k][0] for k in params]
    status = f(*[kinds[k][1] for k in params])
    print("DONE", name, status, lib.polee_last_error(None).decode("utf-8", "replace").replace("\n", " "), flush=True)
"""


def test_null_arguments_are_refused_by_name():
    from polee_amd import _lib
    todo = [(n, k) for n, k in declared_entry_points() if n not in EXEMPT]
    assert len(EXEMPT) <= 5
    assert len(todo) >= 180, len(todo)
    r = subprocess.run([sys.executable, "-c", CHILD, _lib.LIB_PATH, json.dumps(todo)], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    last = [l for l in lines if l.startswith("CALL ")]
    assert r.returncode == 0, ("the child died in", last[-1] if last else None, r.stderr[-2000:])
    done = {}
    for l in lines:
        if l.startswith("DONE "):
            _, name, status, msg = (l.split(" ", 3) + [""])[:4]
            done[name] = (int(status), msg)
    bad = {n: done.get(n) for n, _ in todo if n not in done or done[n][0] != POLEE_ERR_BAD_ARG or not done[n][1].startswith(n + ":")}
    assert not bad, bad


def _definitions():
    """[(file, name, first statement)] of every status-returning polee_* function defined under csrc"""
    out = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")) + glob.glob(os.path.join(CSRC, "*.hpp"))):
        text = open(path).read()
        for m in re.finditer(r'^(?:extern "C" )?polee_status (polee_\w+)\([^;{]*\)\s*\{', text, flags=re.M):
            body = text[m.end():]
            while True:  # (comments in front of the first statement)
                body = body.lstrip()
                if body.startswith("//"):
                    body = body[body.index("\n"):]
                elif body.startswith("/*"):
                    body = body[body.index("*/") + 2:]
                else:
                    break
            out.append((os.path.basename(path), m.group(1), body[:body.index("\n")]))
    return out


def test_every_entry_point_opens_through_one_of_the_three_openers():
    defs = _definitions()
    defined = {name for _, name, _ in defs}
    declared = set(re.findall(r"\bpolee_status\s+(polee_\w+)\s*\(", _headers_text()))
    # (polee_debug_vi_stamps exists in a diagnostic build only and is declared by its user)
    assert declared <= defined, sorted(declared - defined)
    assert len(defs) >= 190, len(defs)
    bad = [(f, n, s) for f, n, s in defs if not s.startswith(("return entry(", "return ctx_entry(", "return host_entry("))]
    assert not bad, bad
    for path in glob.glob(os.path.join(CSRC, "*")):
        if os.path.isfile(path) and not path.endswith((".so", ".o")):
            assert "reg_entry" not in open(path, errors="replace").read(), path
