"""Stream order of include/range_cspfit.h's entry points on a stream that is busy (`-m gpu`), through
range_amd/_cspfit_native.py and the staged-call harness of tests/stream_order.py (imported, not edited; see there).
The header is parsed here with the harness's own expression, and a stream-taking entry point without a case fails.

A step changes the fit's state, so the step cases run with lr = 0 and no weight decay (every parameter keeps its bits,
the moments move); the outputs compared are the loss scalars and the gradient read back right behind the step on the
same stream, as tests/test_gpu_stream_order_headfit.py does."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import cspfit_cases as K
import stream_order as SO
from range_amd import _cspfit_native as cn
from stream_order import Case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HEADER = "range_cspfit.h"
B, BG, N = 65, 63, 90
CASE = "tanh_three"


def header_entry_points():
    """The harness's expression (stream_order.stream_entry_points) on the new header."""
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    with open(os.path.join(inc, HEADER)) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return [m.group(1) for m in re.finditer(r"\b(range_\w+)\s*\(([^()]*)\)\s*;", text)
            if re.search(r"\brange_stream_t\b", m.group(2))]


@functools.lru_cache(maxsize=None)
def _fit():
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cspfit.npz"))
    p = K.case_params(golden, CASE)
    fit = cn.CspFit(DEV)
    fit.begin(p, K.C, p.class_emb)
    return fit


def _inputs(seed):
    rng = np.random.default_rng(seed)
    t = lambda a, d: torch.from_numpy(np.ascontiguousarray(a.astype(d))).to(DEV)      # noqa: E731
    ll = lambda n: np.stack([rng.uniform(-180, 180, n), rng.uniform(-90, 90, n)], axis=1)      # noqa: E731
    return (t(ll(N), np.float64), t(rng.integers(0, N, B), np.int32), t(rng.integers(0, K.C, B), np.int32), t(ll(BG), np.float64))


def _cases():
    kw = dict(max_grid=2, panel_cols=32)

    def grad():
        fit = _fit()
        return _inputs(10), _inputs(11), lambda x, r, y, bg: fit.grad(x, r, y, bg, 0.5, **kw)

    def loss():
        fit = _fit()
        return _inputs(12), _inputs(13), lambda x, r, y, bg: fit.loss(x, r, y, bg, 0.5, want_emb=True)

    def step():
        fit = _fit()

        def call(x, r, y, bg):
            l3 = fit.step(x, r, y, bg, 0.0, weight=0.5, **kw)
            return l3, fit.grad(x, r, y, bg, 0.5)[0]
        return _inputs(14), _inputs(15), call

    def params():
        # the parameters follow what is in flight on the stream: a staged buffer scales the result
        fit = _fit()
        return (torch.full((1,), 2.0, device=DEV),), (torch.full((1,), 3.0, device=DEV),), lambda s: (fit.flat_params() * s,)
    return [Case("cspfit_grad", ("range_cspfit_grad_grid",), grad), Case("cspfit_loss", ("range_cspfit_loss",), loss),
            Case("cspfit_step", ("range_cspfit_step_grid",), step), Case("cspfit_params", ("range_cspfit_params",), params)]


CASES = _cases()
#: the plain calls are one-line forwards to the _grid calls with max_grid = panel_cols = 0 (cspfit_host.h); their cases
#: go through the library's plain symbols directly
PLAIN = ("range_cspfit_grad", "range_cspfit_step")


def _plain_cases():
    def make(name):
        def build():
            fit = _fit()
            lib, h, e = fit.lib, fit._h, fit.engine

            def call(x, r, y, bg):
                l3 = e._empty((3,), torch.float32)
                rows = [h, x.data_ptr(), N, r.data_ptr(), y.data_ptr(), B, bg.data_ptr(), BG, 0.5]
                if name == "range_cspfit_grad":
                    g = e._empty((fit.param_count,), torch.float32)
                    cn._check(lib, lib.range_cspfit_grad(*rows, 0.0, 0, g.data_ptr(), l3.data_ptr(), e._stream()))
                    return g, l3
                cn._check(lib, lib.range_cspfit_step(*rows, 0.0, 0.9, 0.999, 1e-8, 0.0, 0.0, 0, l3.data_ptr(), e._stream()))
                return (l3,)
            return _inputs(20), _inputs(21), call
        return build
    return [Case(name[len("range_"):] + "_plain", (name,), make(name)) for name in PLAIN]


CASES += _plain_cases()


def test_every_stream_taking_entry_point_of_the_header_has_a_case():
    """Needs no GPU work: the header against the case table."""
    names = header_entry_points()
    assert len(names) == 6 and HEADER not in SO.HEADERS
    covered = {n for case in CASES for n in case.covers}
    assert not sorted(set(names) - covered), f"entry points with a range_stream_t parameter and no case: {sorted(set(names) - covered)}"
    assert not sorted(covered - set(names)), f"cases for entry points the header does not declare: {sorted(covered - set(names))}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_call_orders_on_a_busy_stream(case):
    real, decoy, call = case.build()
    SO.run_staged(case.name, DEV, real, decoy, call, blocks=case.blocks)
