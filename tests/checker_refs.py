"""References for the checkerboard task's nearest-support scan (range_amd/csrc/checker_kernel.h), numpy on
the host: a float64 restatement of the reference's haversine term in its expression order, laid out as the
kernel lays its work out (support tiles dealt round-robin to chunks, a merge of the chunks' winners) so that
defects of the selection can be planted; and the same quantities in long double.

THE DISTANCE BOUND (derived, not measured; eps = 2^-52).  Two evaluations of
    a = sin(dlat/2)^2 + (cos(lat1) cos(lat2)) sin(dlon/2)^2,      c = 2 atan2(sqrt(a), sqrt(1 - a))
from the same float64 radians differ only through their sin / cos / atan2: dlon, dlat and their halves are
single IEEE operations on equal inputs, hence equal bit for bit.  Grant each side 4 ulp on sin and cos (the
OpenCL conformance bound the device library is built to; glibc's are below 1 ulp), i.e. 8 eps relative between
the sides per trigonometric value.  Then, every product and the sum (of non-negative terms) adding one more
eps between the sides:  sin^2: 17 eps;  cos cos: 17 eps;  their product with sin^2: 35 eps;  a: 36 eps
relative.  sqrt halves it (+ eps): y = sqrt(a) differs by 19 eps relative, x = sqrt(1 - a) by
(18 a / (1 - a) + 1) eps relative.  For theta = atan2(y, x) with x^2 + y^2 = 1, |d theta| <= x y (rel y + rel x)
= sqrt(a (1 - a)) * 20 eps + 18 eps a^(3/2) / sqrt(1 - a); atan2 itself 6 ulp + 1 ulp between the sides, rounded
up to 10 eps relative to leave room for the terms dropped as second order.  With sqrt(a) = sin(c/2),
sqrt(1 - a) = cos(c/2):

    |c_1 - c_2|  <=  eps * (20 sin c + 36 sin^2(c/2) tan(c/2) + 10 c)             = dist_bound(c)

The middle term is the 1 / sqrt(1 - a) growth when the nearest point is far (c -> pi).  For a nearest
neighbour at c = 0.02 rad the bound is 0.6 eps.  INDICES: the winner is safe from the 36 eps on a - 18 eps on a
small c - whenever the runner-up's distance is relatively 1e-9 farther (GAP_MIN; asserted on the restatement
before any index is compared).

Against an EXACT evaluation (long double here) the rounding of dlon and dlat is no longer common to both sides:
half an ulp of an argument of at most pi (dlon / 2 across the antimeridian) or pi / 2 (dlat / 2) moves the sine
by as much in absolute terms, and with |sin(dlat/2)|, sqrt(cos cos) |sin(dlon/2)| <= sqrt(a) that is at most
1.5 pi eps / cos(c/2) on c: argument_bound.  It is inherent in the reference's formula, not in an implementation.

Statistics (mean, std of n distances through numpy's own reductions on both sides): the inputs' differences
enter by at most their largest (the mean is an average; the standard deviation is the 2-norm of the centred
vector over sqrt(n), and centring does not lengthen a vector); numpy's pairwise sums and the subtraction of the
mean add at most (log2 n + 8) eps of the mean: stat_bound."""
import numpy as np

EPS = 2.0 ** -52
TILE = 256            # host_plan.h: CHECKER_TILE (tests/native/checker_plan.cpp prints it; test_checker_cpu compares)
GAP_MIN = 1e-9
DEFECTS = ("f32trig", "nocos1", "lasttie", "mergeidx")


def dist_bound(c):
    c = np.asarray(c, dtype=np.float64)
    return EPS * (20.0 * np.sin(c) + 36.0 * np.sin(c / 2) ** 2 * np.abs(np.tan(c / 2)) + 10.0 * c)


def argument_bound(c):
    return EPS * 1.5 * np.pi / np.cos(np.asarray(c, dtype=np.float64) / 2)


def stat_bound(dists, scale=1.0):
    """Bound on the mean and on the standard deviation of ``scale * dists`` between the two sides."""
    d = np.asarray(dists, dtype=np.float64)
    return scale * (dist_bound(d).max() + (np.log2(len(d)) + 8) * EPS * d.mean()) * (1 + 4 * EPS)


def term(q_deg, s_deg, defect=None, dtype=np.float64):
    """(Q,2), (S,2) (lon, lat) degrees -> the (Q,S) haversine terms a."""
    q, s = np.radians(np.asarray(q_deg, dtype=np.float64)).astype(dtype), np.radians(np.asarray(s_deg, dtype=np.float64)).astype(dtype)
    lon1, lat1, lon2, lat2 = q[:, 0], q[:, 1], s[:, 0], s[:, 1]
    dlon = lon2[None, :] - lon1[:, None]
    dlat = lat2[None, :] - lat1[:, None]
    sin = np.sin
    if defect == "f32trig":
        sin = lambda x: np.sin(x.astype(np.float32)).astype(np.float64)     # noqa: E731
    c1 = np.ones_like(lat1) if defect == "nocos1" else np.cos(lat1)
    return sin(dlat / 2) ** 2 + c1[:, None] * np.cos(lat2)[None, :] * sin(dlon / 2) ** 2


def distance(a):
    return 2 * np.arctan2(np.sqrt(a), np.sqrt(1 - a))


def nearest(q_deg, s_deg, exclude_self=False, tile=TILE, chunks=1, defect=None):
    """-> (idx (Q,) int64: -1 without a valid pair, dist (Q,) float64: NaN there), selected as the kernel selects:
    per chunk (tiles y, y + chunks, ...) the smallest a, lowest index first; then the chunks' winners merged on
    (a, index).  A NaN a never wins."""
    with np.errstate(invalid="ignore"):
        a = term(q_deg, s_deg, defect)
    Q, S = a.shape
    if exclude_self:
        assert Q == S
        a[np.arange(Q), np.arange(Q)] = np.nan
    a = np.where(np.isnan(a), np.inf, a)               # (a valid a is at most about 1)
    n_tiles = -(-S // tile)
    chunks = max(1, min(chunks, n_tiles))
    best, best_j = np.full(Q, np.inf), np.full(Q, -1, dtype=np.int64)
    rows = np.arange(Q)
    for y in range(chunks):
        cols = np.concatenate([np.arange(t * tile, min(S, (t + 1) * tile)) for t in range(y, n_tiles, chunks)])
        sub = a[:, cols]
        k = sub.shape[1] - 1 - np.argmin(sub[:, ::-1], axis=1) if defect == "lasttie" else np.argmin(sub, axis=1)
        av, jv = sub[rows, k], cols[k]
        valid = np.isfinite(av)
        if defect == "mergeidx":
            take = valid & (av <= best)
        else:
            take = valid & ((best_j < 0) | (av < best) | ((av == best) & (jv < best_j)))
        best, best_j = np.where(take, av, best), np.where(take, jv, best_j)
    with np.errstate(invalid="ignore"):
        dist = np.where(best_j >= 0, distance(np.where(best_j >= 0, best, 0.0)), np.nan)
    return best_j, dist


def nearest_longdouble(q_deg, s_deg):
    """Arg-min and minimum of the distance itself in long double, from the same float64 radians."""
    a = term(q_deg, s_deg, dtype=np.longdouble)
    c = distance(a)
    return c.argmin(axis=1), c.min(axis=1)


def relative_gap(q_deg, s_deg, exclude_self=False):
    """Per query (d2 - d1) / d2 of the restatement's two smallest distances (S >= 2; inf where d2 is 0)."""
    c = distance(term(q_deg, s_deg))
    if exclude_self:
        c[np.arange(len(c)), np.arange(len(c))] = np.inf
    part = np.partition(c, 1, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(part[:, 1] > 0, (part[:, 1] - part[:, 0]) / part[:, 1], np.inf)


def assert_dist_close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err, bound = np.abs(got[ok] - want[ok]), dist_bound(want[ok])
    assert (err <= bound).all(), f"distance off by up to {(err / np.maximum(bound, 1e-300)).max():.2f} of the bound"
    return float((err / np.maximum(bound, 1e-300)).max()) if ok.any() else 0.0


def random_points(n, seed):
    """n points uniform on the sphere, (lon, lat) degrees."""
    v = np.random.default_rng(seed).normal(size=(3, n))
    return np.stack([np.rad2deg(np.arctan2(v[1], v[0])), np.rad2deg(np.arctan2(v[2], np.hypot(v[0], v[1])))], axis=1)


def tie_case(tile):
    """70 queries and 3 * tile + 5 supports in which the nearest point of each of the first 8 queries (the query
    itself: a = 0) appears four times: at 8 + i, again in the same tile, and in the two following tiles - other
    chunks when the support is split.  numpy.argmin answers 8 + i."""
    q = random_points(70, 21)
    s = random_points(3 * tile + 5, 22)
    for i in range(8):
        for j in (8 + i, tile // 2 + i, tile + 3 * i, 2 * tile + 2 + i):
            s[j] = q[i]
    return q, s
