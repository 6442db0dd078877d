#!/usr/bin/env python3
"""The Python binding's surface as one JSON document: what `binding.NAME` offers, without loading the library.

    python tools/binding_api.py > tests/binding_api.json     (recorded once, from the commit the surface is to be held to)

tests/test_binding_api_cpu.py rebuilds the document and compares it with the recorded one: a refactor of the binding may add
names and must leave every recorded one as it was.  Types are named by __name__ (c_int, LP_Watch, c_void_p), never by repr,
so the document does not say which module of the package a name lives in."""
import ctypes as C
import hashlib
import importlib
import inspect
import json
import re
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _callable(fn) -> list:
    """[signature, SHA-1 of the docstring] of a function; a default that prints with its address (a lambda) prints without it."""
    doc = inspect.getdoc(fn)
    return [re.sub(r" at 0x[0-9a-f]+", "", str(inspect.signature(fn))), hashlib.sha1(doc.encode()).hexdigest() if doc else None]


def _type(t) -> str:
    return "None" if t is None else t.__name__


def _constant(v) -> bool:
    return isinstance(v, (int, float, str)) or (isinstance(v, tuple) and all(_constant(e) for e in v))


def document() -> dict:
    B = importlib.import_module("beamforming-lk_amd").binding
    names = {k: v for k, v in vars(B).items() if not (k.startswith("__") and k.endswith("__"))}
    classes = {k: v for k, v in names.items() if inspect.isclass(v)}
    structures = {k: v for k, v in classes.items() if issubclass(v, C.Structure)}
    plain = {k: v for k, v in classes.items() if k not in structures and not issubclass(v, C._Pointer)}
    tables = {k: v for k, v in names.items() if k.endswith("_SIGNATURES") and isinstance(v, dict)}
    return {
        "names": sorted(names),
        "functions": {k: _callable(v) for k, v in names.items() if inspect.isfunction(v)},
        "engine": {k: _callable(v) for k, v in vars(B.Engine).items() if inspect.isfunction(v)},
        "classes": {k: {"init": _callable(v.__init__), "doc": _callable(v)[1], "bases": [b.__name__ for b in v.__bases__],
                        "methods": sorted(m for m, f in vars(v).items() if inspect.isfunction(f))} for k, v in plain.items()},
        "pointers": {k: _type(v) for k, v in classes.items() if issubclass(v, C._Pointer)},
        "signatures": {t: {name: [_type(res), [_type(a) for a in args]] for name, (res, args) in table.items()} for t, table in tables.items()},
        "all_signatures": [next(t for t, table in tables.items() if table is entry) for entry in B._ALL_SIGNATURES],
        "structures": {k: {"sizeof": C.sizeof(v), "fields": [[f, _type(t), getattr(v, f).offset, getattr(v, f).size] for f, t in v._fields_]}
                       for k, v in structures.items()},
        "dtypes": {k: {"descr": v.descr, "itemsize": v.itemsize} for k, v in names.items() if isinstance(v, np.dtype)},
        "constants": {k: v for k, v in names.items() if k.isupper() and _constant(v)},
    }


def dump(doc: dict, out) -> None:
    """The document with one entry a line (one entry point a line in "signatures"): a change shows as the lines it touches."""
    def entries(value: dict, depth: int) -> str:
        pad = " " * (depth + 1)
        rows = [f"{pad}{json.dumps(k)}: " + (entries(v, depth + 1) if depth == 1 and isinstance(v, dict) else json.dumps(v, sort_keys=True))
                for k, v in sorted(value.items())]
        return "{\n" + ",\n".join(rows) + "\n" + " " * depth + "}"
    rows = [f' {json.dumps(k)}: ' + (entries(v, 1) if k == "signatures" else entries(v, 2) if isinstance(v, dict) else json.dumps(v))
            for k, v in sorted(doc.items())]
    out.write("{\n" + ",\n".join(rows) + "\n}\n")


if __name__ == "__main__":
    dump(document(), sys.stdout)
