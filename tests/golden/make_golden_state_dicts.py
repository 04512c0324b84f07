"""Generates tests/golden/refmodels_state_dict_shapes.json: the state-dict key names and shapes of the REFERENCE's own
models.FlowNet2C and models.FlowNet2 (models.py:120, :14), built from where they lie.  Dev container only (needs the reference
checkout and this repo's built extension modules, which the reference's networks/ wrappers import):
    python tests/golden/make_golden_state_dicts.py [REFERENCE_ROOT]
tests/test_harness.py checks harness.FlowNet2C / harness.FlowNet2 against the fixture everywhere, and the fixture against the
live classes where the reference checkout exists."""
import importlib
import json
import os
import sys
from types import SimpleNamespace

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"


def main():
    sys.path[:0] = [REF, os.path.join(ROOT, "flownet2-pytorch_amd")]   # the reference's models + networks, OUR correlation_cuda etc.
    models = importlib.import_module("models")
    args = SimpleNamespace(rgb_max=255.0, fp16=False)
    table = {name: {k: list(v.shape) for k, v in getattr(models, name)(args).state_dict().items()} for name in ("FlowNet2C", "FlowNet2")}
    with open(os.path.join(OUT, "refmodels_state_dict_shapes.json"), "w") as f:   # one key per line, in state-dict order
        f.write("{\n" + ",\n".join(json.dumps(name) + ": {\n" + ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sd.items())
                                   + "\n}" for name, sd in table.items()) + "\n}\n")
    print("wrote", {k: len(v) for k, v in table.items()})


if __name__ == "__main__":
    main()
