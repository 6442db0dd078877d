"""ctypes binding of libawpu_hip.so (include/awpu_hip.h): the one name everybody imports.

Plumbing only: it loads the in-tree HIP library and forwards to the C ABI.  There is no
Python or CPU implementation of the sweep behind it -- if the library cannot be built or
loaded, importing a compute entry point raises.

Nothing is defined here.  The code is in four modules, each importing only those before it:
abi (the C ABI as ctypes, load() and the argument helpers), results (the result classes), rules
(geometry and the headers' rules on the host, no handle) and engine (Engine).  Every name of
theirs, private ones included, is also a name of this module, and is the same object.
"""
from __future__ import annotations

from . import abi, engine, results, rules

# (_lib is left out: load() and loaded_library() rebind it in abi, and a copy made here would go stale)
globals().update({name: value for module in (abi, results, rules, engine) for name, value in vars(module).items()
                  if not name.startswith("__") and name != "_lib"})


def __getattr__(name: str):
    """binding._lib is abi's, read when asked for: None until load(), the stand-in within loaded_library()."""
    if name == "_lib":
        return abi._lib
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
