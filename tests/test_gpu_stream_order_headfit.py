"""Stream order of include/range_headfit.h's entry points on a stream that is busy (`-m gpu`), through
range_amd/_headfit_native.py and the staged-call harness of tests/stream_order.py (imported, not edited; see there).
The header is the sixth public one: it is parsed here with the harness's own expression, and a stream-taking entry
point without a case fails.

A step changes the fit's state, so a staged step cannot be repeated from the same weights without ``begin`` (which
synchronises).  The step cases therefore run with lr = 0 and no weight decay: W keeps its bits (W - 0 * m / denom),
the moments move, and the outputs compared are the loss scalars - they depend on the step's inputs, which is what the
staging varies - and the gradient read back right behind the step on the same stream."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import stream_order as SO
from range_amd import _headfit_native as hn
from stream_order import Case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HEADER = "range_headfit.h"
B, BG, C, F, N = 65, 63, 129, 40, 90


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
    fit = hn.HeadFit(DEV)
    W = (np.random.default_rng(1).standard_normal((C, F)) * 0.2).astype(np.float32)
    fit.begin(C, F, W)
    return fit


def _inputs(seed):
    rng = np.random.default_rng(seed)
    t = lambda a, d: torch.from_numpy(np.ascontiguousarray(a.astype(d))).to(DEV)      # noqa: E731
    return (t(rng.standard_normal((N, F)) * 0.7, np.float32), t(rng.integers(0, N, B), np.int32),
            t(rng.integers(0, C, B), np.int32), t(rng.standard_normal((BG, F)) * 0.7, np.float32))


def _cases():
    def grad(grid):
        def build():
            fit = _fit()
            kw = dict(max_grid=2, panel_cols=64) if grid else {}
            return _inputs(10), _inputs(11), lambda x, r, y, bg: fit.grad(x, r, y, bg, 0.5, **kw)
        return build

    def loss(grid):
        def build():
            fit = _fit()
            kw = dict(max_grid=2, panel_cols=64) if grid else {}
            return _inputs(12), _inputs(13), lambda x, r, y, bg: (fit.loss(x, r, y, bg, 0.5, **kw),)
        return build

    def step(grid):
        def build():
            fit = _fit()
            kw = dict(max_grid=2, panel_cols=64) if grid else {}

            def call(x, r, y, bg):
                l3 = fit.step(x, r, y, bg, 0.0, weight=0.5, **kw)
                return l3, fit.grad(x, r, y, bg, 0.5)[0]
            return _inputs(14), _inputs(15), call
        return build

    def weights():
        # the weights follow what is in flight on the stream: a staged buffer scales the result
        fit = _fit()
        return (torch.full((1,), 2.0, device=DEV),), (torch.full((1,), 3.0, device=DEV),), lambda s: (fit.weights() * s,)
    return [Case("headfit_grad", ("range_headfit_grad_grid",), grad(True)), Case("headfit_loss", ("range_headfit_loss_grid",), loss(True)),
            Case("headfit_step", ("range_headfit_step_grid",), step(True)), Case("headfit_weights", ("range_headfit_weights",), weights)]


CASES = _cases()
#: the plain calls are one-line forwards to the _grid calls with max_grid = panel_cols = 0 (headfit_host.h); their
#: cases go through the library's plain symbols directly
PLAIN = {"range_headfit_grad": "range_headfit_grad_grid", "range_headfit_loss": "range_headfit_loss_grid",
         "range_headfit_step": "range_headfit_step_grid"}


def _plain_cases():
    def make(name):
        def build():
            fit = _fit()
            lib, h, e = fit.lib, fit._h, fit.engine

            def call(x, r, y, bg):
                l3 = e._empty((3,), torch.float32)
                rows = [h, x.data_ptr(), N, r.data_ptr(), y.data_ptr(), B, bg.data_ptr(), BG, 0.5]
                if name == "range_headfit_grad":
                    dW = e._empty((C, F), torch.float32)
                    hn._check(lib, lib.range_headfit_grad(*rows, dW.data_ptr(), l3.data_ptr(), e._stream()))
                    return dW, l3
                if name == "range_headfit_loss":
                    hn._check(lib, lib.range_headfit_loss(*rows, l3.data_ptr(), e._stream()))
                    return (l3,)
                hn._check(lib, lib.range_headfit_step(*rows, 0.0, 0.9, 0.999, 1e-8, 0.0, l3.data_ptr(), e._stream()))
                return (l3,)
            return _inputs(20), _inputs(21), call
        return build
    return [Case(name[len("range_"):] + "_plain", (name,), make(name)) for name in PLAIN]


CASES += _plain_cases()


def test_every_stream_taking_entry_point_of_the_header_has_a_case():
    """Needs no GPU work: the header against the case table."""
    names = header_entry_points()
    assert len(names) == 7 and HEADER not in SO.HEADERS
    covered = {n for case in CASES for n in case.covers}
    assert not sorted(set(names) - covered), f"entry points with a range_stream_t parameter and no case: {sorted(set(names) - covered)}"
    assert not sorted(covered - set(names)), f"cases for entry points the header does not declare: {sorted(covered - set(names))}"


def test_the_harness_exposes_a_stale_read():
    assert SO.control_exposes_stale_read(DEV), "no stream exposed the stand-in's stale read: the staging shows nothing here"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_call_orders_on_a_busy_stream(case):
    real, decoy, call = case.build()
    SO.run_staged(case.name, DEV, real, decoy, call, blocks=case.blocks)
