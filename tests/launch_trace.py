"""The recorder of the launch-trace tests (tests/test_volume_launch_trace_host.py, tests/test_edm_sampler_trace_host.py): what a
record holds and how a trace is canonicalised, digested and dumped.  Not a test module."""
import collections
import hashlib
import inspect
import json
import os
import tempfile

import numpy as np
import torch


def f32(v):
    v = float(np.float32(v))
    return v if np.isfinite(v) else str(v)


class Recorder:
    def __init__(self):
        self.trace, self._tags, self._seen, self._alive = [], {}, collections.Counter(), []

    def tag(self, t, role):
        """The tag of the storage ``t`` lives in, made from ``role`` at first sight.  Every tagged tensor is kept alive, so no later
        allocation can take its address."""
        key = t.untyped_storage().data_ptr()
        if key not in self._tags:
            self._tags[key] = f"{role}#{self._seen[role]}"
            self._seen[role] += 1
            self._alive.append(t)
        return self._tags[key]

    def describe(self, v, role):
        if v is None or isinstance(v, (bool, str)):
            return v
        if isinstance(v, (int, np.integer)):
            return int(v)
        if isinstance(v, (float, np.floating)):
            return f32(v)
        if isinstance(v, np.ndarray):
            return {'host': v.tolist()}
        if torch.is_tensor(v):
            if role.endswith(('.slot', '.taps')):
                return {'shape': list(v.shape), 'dtype': str(v.dtype), 'sha': hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest()[:16]}
            if not v.is_floating_point():
                return {'index': v.tolist()}
            return {'t': self.tag(v, role), 'shape': list(v.shape), 'dtype': str(v.dtype), 'off': v.storage_offset()}
        if isinstance(v, (tuple, list)):
            return [self.describe(e, role) for e in v]
        if callable(v):
            return 'callable'
        return str(v)

    def record(self, op, args, result=None):
        """Append the call; tag what it returned (``result`` tensors the call did not receive are fresh ones) and hand it back."""
        rec = {'op': op, **{k: self.describe(v, f"{op}.{k}") for k, v in args.items()}}
        rec['->'] = self.describe(result, op)
        self.trace.append(rec)
        return result


def zeros(*shape):
    return torch.zeros(tuple(int(s) for s in shape), dtype=torch.float32)


class RecordingOps:
    """Stands in for ``diffusioniqt_amd.ops`` inside a module: every call is bound to the real op's signature (so positional / keyword
    spelling and explicit defaults do not matter), recorded, and answered by ``returns[name](bound arguments)``; an op that is not in
    ``returns`` is an AttributeError."""

    def __init__(self, rec, returns):
        from diffusioniqt_amd import ops
        self._rec, self._real, self._returns = rec, ops, returns

    def __getattr__(self, name):
        if name not in self._returns:
            raise AttributeError(f"the launch trace has no stand-in for ops.{name}")
        sig = inspect.signature(getattr(self._real, name))

        def op(*args, **kw):
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            return self._rec.record(name, bound.arguments, self._returns[name](bound.arguments))
        return op


def canonical(trace):
    return json.dumps(trace, sort_keys=True, separators=(',', ':'))


def dump(name, trace, where=None, prefix='launch_trace_'):
    where = where or tempfile.mkdtemp(prefix=prefix)
    os.makedirs(where, exist_ok=True)
    path = os.path.join(where, name + '.json')
    with open(path, 'w') as f:
        f.write('[\n' + ',\n'.join(canonical([r])[1:-1] for r in trace) + '\n]\n')       # one record per line: diff-able
    return path
