"""The reference kernels' answers without the reference: tests/golden/make_golden_oracle_vs_ref.py runs the calls of
tests/test_oracle_vs_ref.py through Recorder(Oracle(ref=True)) (the reference's device code under the CPU SIMT shim) and stores
every result in tests/golden/oracle_vs_ref_calls.npz; where oracle/_ref/ has not been built, Replay answers the same calls
from that file.  A call is identified by the operation's name and its exact arguments (array bytes, dtype, shape; scalars)."""
import hashlib

import numpy as np


def call_key(op, args):
    h = hashlib.sha1(op.encode())
    for a in args:
        if isinstance(a, np.ndarray):
            h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
            h.update(np.ascontiguousarray(a).tobytes())
        else:
            h.update(repr(a).encode())
    return op + "_" + h.hexdigest()[:20]


class Recorder:
    def __init__(self, live):
        self.live, self.calls = live, {}

    def __getattr__(self, op):
        def call(*args):
            out = getattr(self.live, op)(*args)
            outs = out if isinstance(out, tuple) else (out,)
            key = call_key(op, args)
            for i, o in enumerate(outs):
                self.calls["%s.%d%s" % (key, i, "t" if isinstance(out, tuple) else "")] = np.asarray(o)
            return out
        return call

    def save(self, path):
        np.savez_compressed(path, **self.calls)


class Replay:
    def __init__(self, path):
        d = np.load(path)
        self.calls = {k: d[k] for k in d.files}

    def __getattr__(self, op):
        def call(*args):
            key = call_key(op, args)
            names = sorted((k for k in self.calls if k.startswith(key + ".")), key=lambda k: int(k.split(".")[1].rstrip("t")))
            assert names, "no recorded reference answer for this %s call (rerun tests/golden/make_golden_oracle_vs_ref.py)" % op
            outs = tuple(self.calls[k] for k in names)
            return outs if names[0].endswith("t") else outs[0]
        return call
