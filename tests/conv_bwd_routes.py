"""Helpers of tests/test_gpu_conv_bwd_routes.py: what one `Trainer.step` asks of the library, call by call.

`trace_step` wraps `libdat.Ctx.call` for the length of one step and records, per call: the phase (forward or backward), the name, the
non-pointer arguments, the fields of every descriptor and which pointer arguments of that call are equal to each other.  `histogram`
condenses a trace into the routes `TrainExecutor.bwd_Conv` chose: a fusion that silently stops firing changes it, while every parity
test still passes.  tests/conv_bwd_routes.json holds the histograms recorded at the commit before the backward was split into plan and
launch.
"""
import collections
import ctypes as C
import json
import os

ROUTES_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_bwd_routes.json')

# position of the output pointer among the arguments of the conv launches the data gradient uses
_OUT_ARG = {'dat_conv3d_fwd': 7, 'dat_conv3d_fwd_sum_mask': 8, 'dat_conv3d_grouped_fwd': 8}
_WGRAD = ('dat_conv3d_wgrad', 'dat_conv3d_wgrad_acc', 'dat_conv3d_grouped_wgrad', 'dat_conv3d_grouped_wgrad_acc')


def _fields(s):
    out = collections.OrderedDict()
    for name, typ in s._fields_:
        v = getattr(s, name)
        if typ is C.c_void_p:                   # an address: only its coincidences are recorded (_aliases)
            continue
        if isinstance(v, (int, float)):
            out[name] = v
        elif isinstance(v, C._Pointer):         # a pointer to another structure (WgradJob.desc)
            out[name] = _fields(v.contents) if v else None
        elif isinstance(v, C.Array):
            out[name] = _array(v)
        elif isinstance(v, C.Structure):
            out[name] = _fields(v)
    return out


def _aliases(s):
    """Which address fields of one structure coincide."""
    ptrs = [getattr(s, n) for n, typ in s._fields_ if typ is C.c_void_p]
    return [[i, j] for i in range(len(ptrs)) for j in range(i + 1, len(ptrs)) if ptrs[i] and ptrs[i] == ptrs[j]]


def _array(a):
    if issubclass(a._type_, C.Structure):
        return [dict(_fields(s), aliases=_aliases(s)) for s in a]
    if a._type_ in (C.c_void_p, C.c_char):       # addresses / opaque bytes: only how many
        return ['%d x %s' % (len(a), a._type_.__name__)]
    return list(a)


def describe(phase, name, args):
    """One call as plain data: no addresses, only which of them coincide."""
    scalars, descs, ptrs = [], [], collections.OrderedDict()
    for k, a in enumerate(args):
        if a is None:
            scalars.append(None)            # a null pointer is a choice (no residual, no bias), not an address
        elif isinstance(a, C.c_void_p):
            if a.value:
                ptrs.setdefault(a.value, []).append(k)
            else:
                scalars.append(None)
        elif isinstance(a, (int, float)):
            scalars.append(a)
        elif isinstance(a, C._SimpleCData):
            scalars.append(a.value)
        elif isinstance(a, C.Array):
            descs.append(_array(a))
        elif hasattr(a, '_obj'):            # byref(structure)
            descs.append(_fields(a._obj))
        else:
            scalars.append(type(a).__name__)
    return {'phase': phase, 'name': name, 'scalars': scalars, 'descs': descs, 'aliases': [v for v in ptrs.values() if len(v) > 1]}


def trace_step(monkeypatch, trainer, lr=0.0):
    """Run `trainer.step(lr)` -> (the executor it returns, [describe(...)] of every library call in order)."""
    from detectandtrack_amd import libdat, training
    calls, phase = [], ['fwd']
    real_call, real_bwd = libdat.Ctx.call, training.TrainExecutor.backward

    def call(self, name, *args):
        calls.append(describe(phase[0], name, args))
        return real_call(self, name, *args)

    def backward(self, *a, **kw):
        phase[0] = 'bwd'
        return real_bwd(self, *a, **kw)
    with monkeypatch.context() as m:
        m.setattr(libdat.Ctx, 'call', call)
        m.setattr(training.TrainExecutor, 'backward', backward)
        ex = trainer.step(lr)
    return ex, calls


def histogram(calls):
    h = collections.OrderedDict((k, collections.OrderedDict()) for k in ('dgrad', 'relu_bias_bwd', 'wgrad'))
    h['sum_mask'] = h['wgrad_finish_batch'] = 0
    h['acc_batch_jobs'] = []

    def bump(d, key):
        d[key] = d.get(key, 0) + 1
    for c in calls:
        name = c['name']
        if c['phase'] == 'bwd' and name in _OUT_ARG:
            aliased = any(_OUT_ARG[name] in grp for grp in c['aliases'])
            bump(h['dgrad'], 'res_mode %d, out %s' % (c['descs'][0]['res_mode'], 'aliases an input' if aliased else 'is its own tensor'))
            h['sum_mask'] += name == 'dat_conv3d_fwd_sum_mask'
        elif name == 'dat_relu_bias_bwd':
            bump(h['relu_bias_bwd'], 'relu %d' % c['scalars'][-1])
        elif name in _WGRAD:
            bump(h['wgrad'], name)
        elif name == 'dat_conv3d_wgrad_acc_batch':
            h['acc_batch_jobs'].append(len(c['descs'][0]))
        elif name == 'dat_wgrad_finish_batch':
            h['wgrad_finish_batch'] += 1
    for k in ('dgrad', 'relu_bias_bwd', 'wgrad'):
        h[k] = collections.OrderedDict(sorted(h[k].items()))
    return h


def load_recorded():
    with open(ROUTES_JSON) as f:
        return json.load(f)
