"""The seed walks behind every GPU case of the active-set box-QP tests, pinned: tests/golden/box_qp_walks.json records, per walk
the GPU files call, the seeds it chooses and of each chosen problem's reference run the status, the solve count, a SHA-256 over
the trace's acts and changed counts, a SHA-256 over the float64 bytes of x, z, y, lam and the smallest margin as float.hex; for
one problem of each form also a SHA-256 over the reference gradients for a fixed upstream.  The manifest was recorded before the
three references of the iteration became box_qp_active_ref, so equality here - decisions exactly, floats bit for bit - says
that the reference the device is held to did not move."""
import hashlib
import json
import os

import numpy as np
import pytest

import box_qp_huber_ref as R
import box_qp_pdas_ref as D
import box_qp_soft_ref as SR

MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_qp_walks.json")
COLD = [(S, C, K) for S, C in D.SHAPES for K in D.COLD_K]
CONSTRUCTED = [(S, C, K) for S, C in D.SHAPES for K in D.CONSTRUCTED_K]
MIXED_F32 = [(S, C, SR.MIXED_F32_K) for S, C in D.SHAPES]
LAYER = SR.LAYER_CASES
GRADS_AT = (6, 3, 9)                              # the problem of each form whose gradients are recorded


def runs_of(ps):
    return [(p["seed"], p["run"]) for p in ps if p is not None]


def weight_batch_runs():
    seed, _, _, runs = SR.weight_batch_box()
    return [(seed, run) for run in runs]


WALKS = {}
for S, C, K in COLD:
    WALKS["control/%d-%d-%d" % (S, C, K)] = lambda S=S, C=C, K=K: D.control_box(S, C, K)
    WALKS["soft/%d-%d-%d" % (S, C, K)] = lambda S=S, C=C, K=K: SR.soft_box(S, C, K)
    WALKS["mixed/%d-%d-%d" % (S, C, K)] = lambda S=S, C=C, K=K: SR.mixed_box(S, C, K)
    WALKS["huber/%d-%d-%d" % (S, C, K)] = lambda S=S, C=C, K=K: R.huber_box(S, C, K)
for S, C, K in CONSTRUCTED:
    WALKS["constructed/%d-%d-%d" % (S, C, K)] = lambda S=S, C=C, K=K: D.constructed_cold(S, C, K)
for S, C in D.SHAPES:
    WALKS["control-f32/%d-%d-9" % (S, C)] = lambda S=S, C=C: D.control_box(S, C, 9, f32=True)
for S, C, K in SR.F32_CASES:
    WALKS["soft-f32/%d-%d-%d" % (S, C, K)] = lambda S=S, C=C, K=K: SR.soft_box(S, C, K, f32=True)
    WALKS["huber-f32/%d-%d-%d" % (S, C, K)] = lambda S=S, C=C, K=K: R.huber_box(S, C, K, f32=True)
for S, C, K in MIXED_F32:
    WALKS["mixed-f32/%d-%d-%d" % (S, C, K)] = lambda S=S, C=C, K=K: SR.mixed_box(S, C, K, f32=True)
for S, C, K in LAYER:
    WALKS["mixed-layer/%d-%d-%d" % (S, C, K)] = lambda S=S, C=C, K=K: [SR.mixed_layer_box(S, C, K)]
    WALKS["capped-mixed/%d-%d-%d" % (S, C, K)] = lambda S=S, C=C, K=K: [R.mixed_box(S, C, K)]
for kind in SR.LAYER_BATCHES:
    WALKS["layer-batch/" + kind] = lambda kind=kind: SR.layer_batch(kind)[0]
WALKS["soft-batch/14-7-9"] = lambda: SR.soft_box(*SR.BATCH[:3], count=2)
WALKS["huber-batch/14-7-9"] = lambda: R.huber_box(*SR.BATCH[:3], count=2)
WALKS["weight-batch/14-7-9"] = weight_batch_runs
WALKS["control-long"] = lambda: D.control_box(*D.LONG, sparse=True)
WALKS["soft-long"] = lambda: [SR.soft_long()]
WALKS["mixed-long"] = lambda: [SR.mixed_long()]
WALKS["huber-long"] = lambda: [R.huber_long()]
WALKS["di-trio"] = D.di_trio
WALKS["di-broadcast"] = lambda: [D.di_broadcast()]
WALKS["di-soft-trio"] = SR.di_soft_trio
WALKS["di-soft-pair"] = SR.di_soft_pair
GRADS = {"%s/%d-%d-%d" % ((form,) + GRADS_AT) for form in ("control", "constructed", "soft", "mixed", "huber", "capped-mixed")}


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def grads_of(p, x, lam, xbar, lambar):
    return SR.reference_grads(p, x, lam, xbar, lambar)


def record(got, grads=False):
    """The manifest entry of one walk's result (a list of problems, or of (seed, run) pairs): one record per chosen problem;
    grads: the first problem's reference gradients for a fixed upstream too."""
    pairs = got if got and isinstance(got[0], tuple) else runs_of(got)
    out = []
    for seed, run in pairs:
        trace = run["trace"]
        changed = np.array([-1 if t["changed"] is None else t["changed"] for t in trace], np.int64)
        out.append(dict(seed=seed, status=int(run["status"]), iters=int(run["iters"]),
                        trace=sha([np.asarray(t["act"], np.int8) for t in trace] + [changed]),
                        point=sha([np.asarray(run[k], np.float64) for k in ("x", "z", "y", "lam")]),
                        margin=float(min(t["margin"] for t in trace)).hex()))
    if grads:
        p = got[0]
        rng = np.random.default_rng(0)
        g = grads_of(p, p["run"]["x"], p["run"]["lam"], rng.standard_normal(len(p["run"]["x"])), rng.standard_normal(len(p["run"]["lam"])))
        out[0]["grads"] = sha([np.asarray(g[k], np.float64) for k in sorted(g)])
    return out


def entry(name):
    """The manifest entry of one walk: a list with one record per chosen problem."""
    return record(WALKS[name](), name in GRADS)


with open(MANIFEST) as f:
    WANT = json.load(f)


def test_the_manifest_names_every_walk():
    assert sorted(WANT) == sorted(WALKS)


@pytest.mark.parametrize("name", sorted(WALKS))
def test_walk_is_the_recorded_one(name):
    assert entry(name) == WANT[name]
