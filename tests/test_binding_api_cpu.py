"""The binding's surface against tests/binding_api.json (tools/binding_api.py's document, recorded before Engine's run helpers were
restated): every recorded name is still reachable as binding.NAME and says what it said -- signatures, docstrings, the 131 entry
points' types, structure layouts, record dtypes, constants.  The surface may grow; nothing recorded may go or change.  One kind
of entry is held to its name alone: the eleven run helpers of Engine named in RESTATED, whose arguments are now keywords.  A later
split of binding.py into modules is a pure move if this file still passes."""
import ast
import ctypes as C
import importlib
import inspect
import json
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
import binding_api  # noqa: E402

# Engine's per-run helpers: the recorded signatures took 8 to 25 positional arguments; they now take one run triple and keywords
# (what the public methods pass them is checked on the device, run by run).  Their names stay; nothing else of Engine is exempt.
RESTATED = ("_watch", "_spectral", "_find", "_expose", "_peel_run", "_cohere_run", "_tones_run", "_csm_watch", "_csm_clean_run", "_locate",
            "_listen")
SECTIONS = ("functions", "engine", "classes", "pointers", "signatures", "structures", "dtypes", "constants")


@pytest.fixture(scope="module")
def recorded():
    return json.loads((REPO / "tests" / "binding_api.json").read_text())


@pytest.fixture(scope="module")
def now():
    return json.loads(json.dumps(binding_api.document()))  # (through JSON: tuples compare as the lists the record holds)


def test_the_record_is_the_surface_the_split_started_from(recorded):
    assert len(recorded["names"]) == 213 and len(recorded["functions"]) == 62 and len(recorded["engine"]) == 108
    assert len(recorded["classes"]) + len(recorded["pointers"]) + len(recorded["structures"]) == 33
    assert sum(len(table) for table in recorded["signatures"].values()) == 131


def test_every_recorded_name_is_reachable():
    B = importlib.import_module("beamforming-lk_amd").binding
    recorded = json.loads((REPO / "tests" / "binding_api.json").read_text())
    assert [name for name in recorded["names"] if not hasattr(B, name)] == []


@pytest.mark.parametrize("section", SECTIONS)
def test_nothing_recorded_has_changed(recorded, now, section):
    for name, was in recorded[section].items():
        assert name in now[section], f"{section}: {name} is gone"
        if section == "engine" and name in RESTATED:
            continue
        if section == "signatures":
            for entry, types in was.items():
                assert now[section][name].get(entry) == types, f"{name}: {entry}"
        elif section == "classes":
            assert {k: v for k, v in now[section][name].items() if k != "methods"} == {k: v for k, v in was.items() if k != "methods"}, name
            assert set(was["methods"]) <= set(now[section][name]["methods"]), f"{name}: a method is gone"
        else:
            assert now[section][name] == was, f"{section}: {name}"


def test_load_sets_the_same_tables_in_the_same_order(recorded, now):
    assert now["all_signatures"] == recorded["all_signatures"]


def test_import_and_document_load_no_library():
    """In a fresh interpreter: importing the package and building the document leave the library unloaded (load() is what builds)."""
    code = ("import importlib, sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tools']; "
            "B = importlib.import_module('beamforming-lk_amd').binding; import binding_api; binding_api.document(); "
            "assert B._lib is None; print('unloaded')")
    done = subprocess.run([sys.executable, "-c", code, str(REPO)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip() == "unloaded", done.stderr


# ---- the split: binding.py is a facade over abi, results, rules and engine, each importing only those before it

PACKAGE = "beamforming-lk_amd"
MODULES = ("abi", "results", "rules", "engine")


def _module(name: str):
    return importlib.import_module(f"{PACKAGE}.{name}")


def _tree(name: str) -> ast.Module:
    return ast.parse((REPO / PACKAGE / f"{name}.py").read_text())


def _siblings(name: str) -> set:
    """The modules of the package that <name>.py imports, read from its source (every import in it, at any depth)."""
    found = set()
    for node in ast.walk(_tree(name)):
        if isinstance(node, ast.ImportFrom) and node.level:
            found |= {node.module.split(".")[0]} if node.module else {alias.name for alias in node.names}
        elif isinstance(node, ast.Name):  # (the hyphen keeps the package out of an import statement: the other way to a sibling)
            assert node.id not in ("importlib", "__import__"), f"{name}.py imports by name at line {node.lineno}"
    return found


def test_every_definition_has_one_owner():
    B = _module("binding")
    owned = dict.fromkeys(MODULES, 0)
    for name, value in vars(B).items():
        if name.startswith("__") or not (inspect.isfunction(value) or inspect.isclass(value)) or not value.__module__.startswith(PACKAGE):
            continue
        if inspect.isclass(value) and issubclass(value, C._Pointer):  # (_f32p and its like: made by a call, not by a class statement)
            assert value.__module__ == f"{PACKAGE}.abi" and getattr(_module("abi"), name) is value, name
            continue
        owner =value.__module__.rpartition(".")[2]
        assert owner in MODULES, f"{name} is defined in {value.__module__}"
        assert getattr(_module(owner), name) is value, name
        owned[owner] += 1
    assert owned["engine"] == 1 and B.Engine is _module("engine").Engine and B.Watch is _module("abi").Watch
    assert sum(owned.values()) == 101, owned  # binding.py's top-level functions and classes before the split


def test_each_module_imports_only_those_before_it():
    assert _siblings("abi") == {"_build"}
    assert _siblings("results") == {"abi"}
    assert _siblings("rules") == {"abi", "results"}
    assert _siblings("engine") == {"abi", "results", "rules"}
    assert _siblings("binding") == set(MODULES)


def test_the_facade_defines_nothing():
    """binding.py: a docstring, imports, one statement that re-exports and the __getattr__ that serves _lib."""
    body = _tree("binding").body
    assert isinstance(body[0], ast.Expr) and isinstance(body[0].value, ast.Constant) and isinstance(body[0].value.value, str)
    rest = [node for node in body[1:] if not isinstance(node, (ast.Import, ast.ImportFrom))]
    assert [type(node) for node in rest] == [ast.Expr, ast.FunctionDef], [ast.unparse(node)[:60] for node in rest]
    assert ast.unparse(rest[0].value.func) == "globals().update" and rest[1].name == "__getattr__"


def test_every_name_of_the_modules_is_a_name_of_the_facade():
    B = _module("binding")
    for module in map(_module, MODULES):
        for name, value in vars(module).items():
            if not name.startswith("__") and name != "_lib":
                assert vars(B)[name] is value, f"{module.__name__}.{name}"
    assert "_lib" not in vars(B) and all("_lib" not in vars(_module(m)) for m in MODULES[1:])  # one owner: abi


def test_binding_lib_is_live():
    """binding._lib is abi's at the moment it is read: load() and loaded_library() rebind it there, and no copy goes stale."""
    B = _module("binding")
    real = B.load()
    assert B._lib is real
    sentinel = object()
    with B.loaded_library(sentinel):
        assert B._lib is sentinel and B.load() is sentinel
    assert B._lib is real and B.load() is real
