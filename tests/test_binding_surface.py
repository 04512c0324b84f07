"""The Python surface of the ten pybind modules against its record (tests/golden/binding_surface.json, written by
tests/golden/make_golden_binding_surface.py): the public names, every function's docstring -- under pybind the full signature with
its defaults -- the module's docstring and every integer attribute.  No GPU: importing a module launches nothing."""
import importlib
import json
import os

import pytest

from conftest import GOLDEN

import build

RECORD = os.path.join(GOLDEN, "binding_surface.json")


def surface(name):
    mod = importlib.import_module(name)
    public = sorted(n for n in dir(mod) if not n.startswith("_"))
    attrs = {n: getattr(mod, n) for n in public}
    return {"names": public, "doc": mod.__doc__,
            "functions": {n: a.__doc__ for n, a in attrs.items() if callable(a)},
            "integers": {n: a for n, a in attrs.items() if isinstance(a, int) and not isinstance(a, bool)}}


def test_the_record_covers_the_ten_modules():
    assert sorted(json.load(open(RECORD))) == sorted(build.MODULES) and len(build.MODULES) == 10


@pytest.mark.parametrize("name", build.MODULES)
def test_module_surface_is_the_recorded_one(name):
    want, got = json.load(open(RECORD))[name], surface(name)
    assert got["names"] == want["names"]
    assert got["doc"] == want["doc"]
    assert got["integers"] == want["integers"]
    assert sorted(got["functions"]) == sorted(want["functions"]) and set(got["functions"]) | set(got["integers"]) == set(got["names"])
    for fn in want["functions"]:
        assert got["functions"][fn] == want["functions"][fn], fn
