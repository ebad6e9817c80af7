"""Stream order of the side libraries' entry points - include/range_probe.h, range_map.h, range_cluster.h and
range_neighbors.h with its KDE calls - on a stream that is busy (`-m gpu`), through their native wrappers and the
staged-call harness of tests/stream_order.py (see there and tests/test_gpu_stream_order.py).  The shapes are the
small ones of these libraries' own GPU tests.  The calls their headers state as synchronising - the probe's solve
(it reads the factorisation status) and the cluster linkage (a 4-byte read per round) - are staged as ``blocks``;
the install calls (``set_*``, ``reserve``) take no stream and are not here.  The coverage check that compares these
tables with the headers is tests/test_gpu_stream_order.py::test_every_stream_taking_entry_point_has_a_case."""
import functools

import numpy as np
import pytest
import torch

import stream_order as SO
from range_amd._native import CSP_IMG_F32, _check
from stream_order import Case

DEV = "cuda:0"


def _dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.from_numpy(a).to(DEV)


def _normal(shape, seed):
    return _dev(np.random.default_rng(seed).standard_normal(shape))


def _two(make, seed):
    """(real,), (decoy,) of one input."""
    return (make(seed),), (make(seed + 1),)


# ---------------------------------------------------------------------------------------------- range_probe.h
@functools.lru_cache(maxsize=None)
def _probe():
    from range_amd import _probe_native
    return _probe_native.ProbeEngine(DEV)


def _probe_cases():
    n, d, c, n_alpha = 300, 20, 3, 2

    def colstats():
        pe = _probe()
        return (*_two(lambda s: _normal((n, d), s), 10), lambda X: pe.colstats(X))

    def scale_rows():
        pe = _probe()
        perm = _dev(np.random.default_rng(1).permutation(n)[:200].astype(np.int64))
        scale, offset, shift = (_normal((d,), s) for s in (2, 3, 4))
        return (*_two(lambda s: _normal((n, d), s), 12), lambda X: (pe.scale_rows(X, perm, scale, offset, shift),))

    def onehot():
        pe = _probe()
        shift = _normal((c,), 5)
        code = lambda s: _dev(np.random.default_rng(s).integers(0, c, n), np.int32)      # noqa: E731
        return (*_two(code, 14), lambda cd: (pe.onehot(cd, c, 0, shift),))

    def gemm():
        pe = _probe()
        real, decoy = (_normal((50, 30), 16), _normal((30, 40), 17)), (_normal((50, 30), 18), _normal((30, 40), 19))
        return real, decoy, lambda A, B: (pe.gemm(A, B), pe.gemm(A, A, trans_b=True, lower_only=False))

    def gram():
        pe = _probe()
        real, decoy = (_normal((n, d), 20), _normal((n, c), 21)), (_normal((n, d), 22), _normal((n, c), 23))

        def call(Z, T):
            G, B = torch.zeros((d, d), dtype=torch.float64, device=DEV), pe.empty((d, c))      # (G: the lower triangle is written)
            zsum, tsum = pe.empty(d), pe.empty(c)
            pe.gram(Z, T, G, B, zsum, tsum)
            return G, B, zsum, tsum
        return real, decoy, call

    def sum_parts():
        pe = _probe()
        return (*_two(lambda s: _normal((3, 700), s), 24), lambda P: (pe.sum_parts(P),))

    def solve():
        pe = _probe()
        dd = 70                                   # (two panels of the blocked factorisation)
        zero_d = torch.zeros(dd, dtype=torch.float64, device=DEV)

        def system(seed):                         # (Z centred: zero column sums; the targets' sums give the intercepts)
            M = np.random.default_rng(seed).standard_normal((200, dd))
            return _dev(M.T @ M), _normal((dd, c), seed + 100), _normal((c,), seed + 200)
        return system(26), system(27), lambda G, B, tsum: pe.solve(G, B, zero_d, tsum, [200.0], [0.5, 2.0])

    def scores(seed):
        rng = np.random.default_rng(seed)
        return _dev(rng.standard_normal((n, n_alpha * c))), _dev(rng.standard_normal((n_alpha, c)))

    def r2_sums():
        pe = _probe()

        def inputs(seed):
            T = np.random.default_rng(seed + 50).standard_normal((n, c))
            return (*scores(seed), _dev(T), _dev(T.sum(axis=0)))
        return inputs(28), inputs(29), lambda P, c0, T, ts: (pe.r2_sums(P, c0, T, ts, n_alpha),)

    def accuracy():
        pe = _probe()
        present = torch.ones(c, dtype=torch.int32, device=DEV)

        def inputs(seed):
            return (*scores(seed), _dev(np.random.default_rng(seed + 50).integers(0, c, n), np.int32))
        return inputs(30), inputs(31), lambda P, c0, code: (pe.accuracy(P, c0, code, c, n_alpha, c, present),)
    return [Case("probe_colstats", ("range_probe_colstats",), colstats), Case("probe_scale_rows", ("range_probe_scale_rows",), scale_rows),
            Case("probe_onehot", ("range_probe_onehot",), onehot), Case("probe_gemm", ("range_probe_gemm",), gemm),
            Case("probe_gram", ("range_probe_gram",), gram), Case("probe_sum_parts", ("range_probe_sum_parts",), sum_parts),
            Case("probe_solve", ("range_probe_solve",), solve, blocks=True), Case("probe_r2_sums", ("range_probe_r2_sums",), r2_sums),
            Case("probe_accuracy", ("range_probe_accuracy",), accuracy)]


# ---------------------------------------------------------------------------------------------- range_map.h
MAP_N, MAP_C, MAP_D = 1000, 3, 65


@functools.lru_cache(maxsize=None)
def _map():
    from range_amd import _map_native
    me = _map_native.MapEngine(DEV)
    me.reserve(MAP_N, MAP_C)
    return me


def _map_cases():
    def project():
        me = _map()
        K, mean = _normal((MAP_C, MAP_D), 40), _normal((MAP_D,), 41)
        return (*_two(lambda s: _normal((MAP_N, MAP_D), s), 42), lambda X: (me.project(X, K, mean),))

    def ica_step():
        me = _map()
        W = np.random.default_rng(44).standard_normal((MAP_C, MAP_C))
        return (*_two(lambda s: _normal((MAP_C, MAP_N), s), 45), lambda Y: (me.ica_step(Y, W),))

    def sources():
        me = _map()
        M = np.random.default_rng(47).standard_normal((MAP_C, MAP_C))
        return (*_two(lambda s: _normal((MAP_C, MAP_N), s), 48), lambda Y: (me.sources(Y, M),))

    def equalize():
        me = _map()
        edges = _dev(np.linspace(0.0, 1.0, 257))
        return (*_two(lambda s: _dev(np.random.default_rng(s).random(MAP_N)), 50), lambda x: me.equalize(x, edges))
    return [Case("map_project", ("range_map_project",), project), Case("map_ica_step", ("range_map_ica_step",), ica_step),
            Case("map_sources", ("range_map_sources",), sources), Case("map_equalize", ("range_map_equalize",), equalize)]


# ---------------------------------------------------------------------------------------------- range_cluster.h
CL_N, CL_D = 100, 17


@functools.lru_cache(maxsize=None)
def _cluster():
    from range_amd import _cluster_native
    ce = _cluster_native.ClusterEngine(DEV)
    ce.reserve(CL_N, CL_D)
    return ce


def _cluster_cases():
    def normalize():
        ce = _cluster()
        mask = _dev((np.random.default_rng(60).random(CL_N) < 0.8).astype(np.float64))
        return (*_two(lambda s: _normal((CL_N, CL_D), s), 61), lambda X: ce.normalize(X, mask))

    def unit_rows(seed):
        ce = _cluster()
        E, _ = ce.normalize(_normal((CL_N, CL_D), seed))
        torch.cuda.synchronize()
        return E

    def distances():
        ce = _cluster()
        return (*_two(unit_rows, 63), lambda E: (ce.distances(E),))

    def linkage():
        ce = _cluster()

        def matrix(seed):
            D = ce.distances(unit_rows(seed))
            D.fill_diagonal_(0.0)                 # (+inf there; the linkage never reads the diagonal, and the inputs stay finite)
            torch.cuda.synchronize()
            return D

        def call(D):                              # (D is destroyed: the harness fills the buffer in front of every call)
            merges, heights, _ = ce.linkage(D)
            return merges, heights
        return (*_two(matrix, 65), call)
    return [Case("cluster_normalize", ("range_cluster_normalize",), normalize),
            Case("cluster_distances", ("range_cluster_distances",), distances),
            Case("cluster_linkage", ("range_cluster_linkage",), linkage, blocks=True)]


# ---------------------------------------------------------------------------------------------- range_neighbors.h
NB_N, NB_C, NB_B = 1000, 33, 25


def _images(seed):
    return _dev(np.random.default_rng(seed).random((NB_B, NB_C)).astype(np.float32))


def _labels(seed):
    return _dev(np.random.default_rng(seed).integers(0, NB_C, NB_B), np.int32)


@functools.lru_cache(maxsize=None)
def _neighbors():
    """(engine, the two batches of queries in degrees) - euclidean, with grid cells; 1000 points: four chunks."""
    import neighbor_refs as R
    from range_amd import _neighbors_native as nn
    from range_amd import geo_baselines as gb
    s = R.random_locs(NB_N, 105)
    eng = nn.NeighborEngine(DEV)
    eng.set_neighbors(R.metric_locs(s, False), np.random.default_rng(8).integers(0, NB_C, NB_N), NB_C, False,
                      cells=gb.train_cells(s, 12, 6))
    assert nn.plan(NB_B, NB_N, NB_C)["chunks"] == 4
    return eng, [R.queries_near(s, NB_B, seed) for seed in (155, 156)]


@functools.lru_cache(maxsize=None)
def _kde():
    """(engine, per batch its (q, thr, two_h2)) - haversine, weighted bins."""
    import kde_refs as K
    import neighbor_refs as R
    from range_amd import _neighbors_native as nn
    s, classes, counts, _ = K.sweep_points(205, NB_N, NB_C)
    eng = nn.NeighborEngine(DEV)
    eng.set_kde_points(R.metric_locs(s, True), classes, counts, NB_C, True)
    batches = []
    for seed in (255, 256):
        rows = K.Rows(R.queries_near(s, NB_B, seed), s, True, 64)
        batches.append((_dev(rows.qm), _dev(rows.thr), _dev(rows.two_h2)))
    return eng, batches


def _neighbor_cases():
    from range_amd import _neighbors_native as nn
    from range_amd import geo_baselines as gb

    def queries():
        eng, (qa, qb) = _neighbors()
        return eng, _dev(qa), _dev(qb), _dev(gb.query_cells(qa, 12, 6)), _dev(gb.query_cells(qb, 12, 6))

    def select():
        eng, qa, qb, _, _ = queries()

        def call(q):
            red_k, j_last = eng._empty((NB_B,), torch.float64), eng._empty((NB_B,), torch.int64)
            _check(eng.lib, eng.lib.range_neighbor_select(eng._h, q.data_ptr(), NB_B, 7, red_k.data_ptr(), j_last.data_ptr(), eng._stream()))
            return (red_k, j_last, *eng.neighbor_select(q, 64, max_grid=2))
        return (qa,), (qb,), call

    def rank():
        eng, qa, qb, ca, cb = queries()

        def call(q, qc, lab, img):
            plain = tuple(eng._empty((NB_B,), torch.int32) for _ in range(3))
            _check(eng.lib, eng.lib.range_neighbor_rank(eng._h, q.data_ptr(), None, NB_B, nn.KNN, 64, 0.0, 0.0, 0.0, img.data_ptr(),
                                                        CSP_IMG_F32, lab.data_ptr(), *[t.data_ptr() for t in plain], eng._stream()))
            return (torch.stack(plain), torch.stack(eng.neighbor_rank(q, None, nn.RADIUS, lab, img, thr=49.0)),
                    torch.stack(eng.neighbor_rank(None, qc, nn.CELL, lab, img, pc=2.0, cpc=66.0, chunks=3)))
        return (qa, ca, _labels(70), _images(71)), (qb, cb, _labels(72), _images(73)), call

    def prior():
        eng, qa, qb, ca, cb = queries()

        def call(q, qc):
            plain = eng._empty((NB_B, NB_C), torch.float64)
            _check(eng.lib, eng.lib.range_neighbor_prior(eng._h, q.data_ptr(), None, NB_B, nn.RADIUS, 0, 49.0, 0.0, 0.0, plain.data_ptr(),
                                                         eng._stream()))
            return (plain, *eng.neighbor_prior(q, None, nn.KNN, k=64, want_counts=True),
                    eng.neighbor_prior(None, qc, nn.CELL, pc=2.0, cpc=66.0, chunks=1))
        return (qa, ca), (qb, cb), call

    def kde_rank():
        eng, (ba, bb) = _kde()

        def call(q, thr, h2, lab, img):
            plain = tuple(eng._empty((NB_B,), torch.int32) for _ in range(3))
            _check(eng.lib, eng.lib.range_kde_rank(eng._h, q.data_ptr(), thr.data_ptr(), h2.data_ptr(), NB_B, img.data_ptr(), CSP_IMG_F32,
                                                   lab.data_ptr(), *[t.data_ptr() for t in plain], eng._stream()))
            return torch.stack(plain), torch.stack(eng.kde_rank(q, thr, h2, lab, img, chunks=3))
        return (*ba, _labels(74), _images(75)), (*bb, _labels(76), _images(77)), call

    def kde_prior():
        eng, (ba, bb) = _kde()

        def call(q, thr, h2):
            plain = eng._empty((NB_B, NB_C), torch.float64)
            _check(eng.lib, eng.lib.range_kde_prior(eng._h, q.data_ptr(), thr.data_ptr(), h2.data_ptr(), NB_B, plain.data_ptr(), eng._stream()))
            return (plain, *eng.kde_prior(q, thr, h2, want_sums=True, chunks=3))
        return ba, bb, call
    return [Case("neighbor_select", ("range_neighbor_select", "range_neighbor_select_grid"), select),
            Case("neighbor_rank", ("range_neighbor_rank", "range_neighbor_rank_grid"), rank),
            Case("neighbor_prior", ("range_neighbor_prior", "range_neighbor_prior_grid"), prior),
            Case("kde_rank", ("range_kde_rank", "range_kde_rank_grid"), kde_rank),
            Case("kde_prior", ("range_kde_prior", "range_kde_prior_grid"), kde_prior)]


CASES = _probe_cases() + _map_cases() + _cluster_cases() + _neighbor_cases()


@pytest.fixture(scope="module", autouse=True)
def _release_contexts():
    """The shared contexts live for this module only."""
    yield
    for cached in (_probe, _map, _cluster, _neighbors, _kde):
        cached.cache_clear()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_call_orders_on_a_busy_stream(case):
    real, decoy, call = case.build()
    delay = SO.run_staged(case.name, DEV, real, decoy, call, blocks=case.blocks)
    print(f"{case.name}: delay {delay:.0f} ms, {SO.sleep_cycles_per_ms(DEV):.0f} cycles / ms")
