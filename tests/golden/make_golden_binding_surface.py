"""Generates tests/golden/binding_surface.json: the Python surface of the ten pybind modules as built (public names, docstrings
with their signatures and defaults, integer attributes), read as tests/test_binding_surface.py reads it.  After a build:
    python tests/golden/make_golden_binding_surface.py
The record pins the surface across changes of the binding sources; regenerate it only when a signature is meant to change."""
import json
import os
import sys

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
from test_binding_surface import RECORD, build, surface  # noqa: E402


def main():
    record = {name: surface(name) for name in build.MODULES}
    with open(RECORD, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(RECORD, {name: len(s["names"]) for name, s in record.items()})


if __name__ == "__main__":
    main()
