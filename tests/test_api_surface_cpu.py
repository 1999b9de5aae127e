"""The host face keeps its surface: every public function and class of `api`, and every public method and property of
engine.DMRG2 and engine.CMpo, is reachable under its name with the signature recorded in tests/golden/api_surface.json.

    python tests/test_api_surface_cpu.py --write      regenerates the fixture from the tree it is run in

No library is loaded: the modules are imported and inspected, nothing is called.
"""
import dataclasses
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from hubbardtn_amd import api, engine  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "api_surface.json")
STATE_CLASSES = ("truncdim", "truncbelow", "DMRG2", "DMRG", "IDMRG2", "TDVP2", "TDVP", "CorrectionVector", "InfiniteHamiltonian",
                 "InfiniteMPS", "FiniteMPS", "ThermalMPS", "Environments")


def _entry(obj):
    if not obj.__module__.startswith("hubbardtn_amd"):
        # a standard-library helper visible through an import (dataclasses.field's signature prints object addresses): the name
        # is recorded and must stay reachable, its signature is not this project's to keep
        return {"external": obj.__module__}
    rec = {"signature": str(inspect.signature(obj))}
    if inspect.isclass(obj):
        rec["dataclass"] = dataclasses.is_dataclass(obj)
        if rec["dataclass"]:
            rec["fields"] = [[f.name, None if f.default is dataclasses.MISSING else repr(f.default)] for f in dataclasses.fields(obj)]
    return rec


def _members(cls):
    out = {}
    for name, raw in vars(cls).items():
        if name.startswith("_"):
            continue
        if isinstance(raw, property):
            out[name] = "property"
        elif inspect.isroutine(getattr(cls, name)):
            out[name] = str(inspect.signature(getattr(cls, name)))
    return out


def surface():
    names = {n: _entry(o) for n, o in vars(api).items()
             if not n.startswith("_") and (inspect.isfunction(o) or inspect.isclass(o))}
    return {"api": names, "engine.DMRG2": _members(engine.DMRG2), "engine.CMpo": _members(engine.CMpo)}


def test_recorded_names_and_signatures():
    want, got = json.load(open(FIXTURE)), surface()
    for name, rec in want["api"].items():
        assert hasattr(api, name), f"api.{name} is gone"
        assert got["api"].get(name) == rec, f"api.{name}: {got['api'].get(name)} != {rec}"
    for cls in ("engine.DMRG2", "engine.CMpo"):
        for name, sig in want[cls].items():
            assert got[cls].get(name) == sig, f"{cls}.{name}: {got[cls].get(name)} != {sig}"


def test_state_classes_are_the_ones_of_states():
    from hubbardtn_amd import states
    for name in STATE_CLASSES:
        assert getattr(api, name) is getattr(states, name), name


def test_private_names_other_modules_and_tests_reach_for():
    for name in ("SEED_STEPS", "_save_result", "_load_result", "_ops", "_OPS"):
        assert hasattr(api, name), name


if __name__ == "__main__":
    if "--write" in sys.argv:
        with open(FIXTURE, "w") as f:
            json.dump(surface(), f, indent=1, sort_keys=True)
            f.write("\n")
