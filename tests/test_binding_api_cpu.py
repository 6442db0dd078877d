"""The binding's surface against tests/binding_api.json (tools/binding_api.py's document, recorded before Engine's run helpers were
restated): every recorded name is still reachable as binding.NAME and says what it said -- signatures, docstrings, the 131 entry
points' types, structure layouts, record dtypes, constants.  The surface may grow; nothing recorded may go or change.  One kind
of entry is held to its name alone: the eleven run helpers of Engine named in RESTATED, whose arguments are now keywords.  A later
split of binding.py into modules is a pure move if this file still passes."""
import importlib
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
