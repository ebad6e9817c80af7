"""Temperature sweeps from one scan, CPU side (no GPU): the launch plan of the statistics kernel
(range_amd/csrc/host_plan.h: plan_kept_stats) under sanitizers, the argument logic of ``sweep``
(range_amd/range.py: sweep_plan), the generated code of kept_stats_kernel (range_amd/csrc/pass1_kept.h)
and the sharded plumbing over gloo with a checker engine."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import range_oracle as O
from tools import synth
from range_amd.dist import ShardedRange, shard_rows
from test_dist_cpu import OracleShardEngine, _free_port
from test_temperatures_cpu import SharpOracleShardEngine, _expect64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kept_stats_plan_under_sanitizers(tmp_path):
    """plan_kept_stats: the splits of plan_pass1 (plain, forced, clamped), pairs in groups of <= 8, the
    per-pair shift of plan_temperatures, the workspace - g++ under ASan + UBSan, run on the CPU."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "kept_stats_plan")
    src = os.path.join(REPO, "tests", "native", "kept_stats_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "kept_stats_plan ok" in p.stdout, p.stdout + p.stderr


def test_sweep_plan():
    from range_amd.range import sweep_plan
    # both lists None: today's beta sweep, whatever the rest
    assert sweep_plan("RANGE+", (0.5,), None, None, 12.0, 40.0, 0.5) is None
    assert sweep_plan("RANGE", None, None, None, 15.0) is None
    # RANGE+: defaults of the missing lists, shapes, pairs
    p = sweep_plan("RANGE+", (0, 0.5, 1), (12, 25, 100), (40, 200), 12.0, 40.0, 0.5)
    assert (p.temps, p.geo_temps, p.betas) == ([12.0, 25.0, 100.0], [40.0, 200.0], [0.0, 0.5, 1.0])
    assert p.lead == (3, 2, 3) and p.scan_taus == (12.0, 40.0)
    # H_i at (temps[i], 0): no geographic head; G_j at (12, geo_temps[j]): a head's pair does not depend on the other list
    assert p.pairs == [(12.0, 0.0), (25.0, 0.0), (100.0, 0.0), (12.0, 40.0), (12.0, 200.0)]
    p = sweep_plan("RANGE+", None, (25,), None, 30.0, 20.0, 0.25)
    assert (p.temps, p.geo_temps, p.betas, p.lead) == ([25.0], [20.0], [0.25], (1, 1, 1))
    assert p.pairs == [(25.0, 0.0), (12.0, 20.0)]
    p = sweep_plan("RANGE+", (0.5,), None, (43, 43.5), 30.0, 20.0, 0.25)
    assert (p.temps, p.geo_temps, p.betas, p.lead) == ([30.0], [43.0, 43.5], [0.5], (1, 2, 1))
    assert sweep_plan("RANGE+", None, iter((12.0, 13.0)), None, 12.0, 40.0, 0.5).lead == (2, 1, 1)   # (any iterable)
    # RANGE: temps alone -> (T, B, 1280)
    p = sweep_plan("RANGE", None, (15, 100), None, 15.0)
    assert (p.temps, p.geo_temps, p.betas, p.lead) == ([15.0, 100.0], [], [], (2,))
    assert p.pairs == [(15.0, 0.0), (100.0, 0.0)] and p.scan_taus == (15.0, 0.0)
    with pytest.raises(ValueError, match="RANGE\\+ only"):
        sweep_plan("RANGE", None, (15,), (40,), 15.0)
    with pytest.raises(ValueError, match="RANGE\\+ only"):
        sweep_plan("RANGE", None, None, (40,), 15.0)
    with pytest.raises(ValueError, match="RANGE\\+ only"):
        sweep_plan("RANGE", (0.5,), (15,), None, 15.0)
    with pytest.raises(ValueError, match="RANGE / RANGE\\+"):
        sweep_plan("SatCLIP", None, (15,), None, 15.0)
    # empty lists
    for betas, temps, geo in (((0.5,), (), None), ((0.5,), None, ()), ((), (12,), None), (None, [], [40])):
        with pytest.raises(ValueError, match="must not be empty"):
            sweep_plan("RANGE+", betas, temps, geo, 12.0, 40.0, 0.5)
    with pytest.raises(ValueError, match="must not be empty"):
        sweep_plan("RANGE", None, (), None, 15.0)
    # every value through check_temperatures
    for bad in (0, -1, float("nan"), float("inf"), 1001):
        with pytest.raises(ValueError, match="at most 1000"):
            sweep_plan("RANGE+", None, (12, bad), None, 12.0, 40.0, 0.5)
        with pytest.raises(ValueError, match="geo_temp.*at most 1000"):
            sweep_plan("RANGE+", None, None, (40, bad), 12.0, 40.0, 0.5)
        with pytest.raises(ValueError, match="at most 1000"):
            sweep_plan("RANGE", None, (bad,), None, 15.0)
    assert sweep_plan("RANGE+", None, (1000,), (1000,), 12.0, 40.0, 0.5).pairs == [(1000.0, 0.0), (12.0, 1000.0)]
    # ... its bf16x3 rule included
    assert sweep_plan("RANGE+", None, (43,), (43,), 12.0, 40.0, 0.5, "bf16x3").lead == (1, 1, 1)
    with pytest.raises(ValueError, match="bf16x3"):
        sweep_plan("RANGE+", None, (12, 100), None, 12.0, 40.0, 0.5, "bf16x3")
    with pytest.raises(ValueError, match="bf16x3"):
        sweep_plan("RANGE+", None, None, (200,), 12.0, 40.0, 0.5, "bf16x3")
    assert sweep_plan("RANGE+", None, (12, 100), None, 12.0, 40.0, 0.5, "exact").lead == (2, 1, 1)


def test_sweep_signatures():
    """The keyword arguments exist on every layer and ``betas`` stays the first positional argument."""
    import inspect
    from range_amd import _native
    from range_amd.range import LocationEncoder, ShardedLocationEncoder
    for fn in (LocationEncoder.sweep, ShardedLocationEncoder.sweep):
        sig = inspect.signature(fn)
        assert list(sig.parameters)[:4] == ["self", "coords", "betas", "return_device"]
        assert sig.parameters["temps"].kind == sig.parameters["geo_temps"].kind == inspect.Parameter.KEYWORD_ONLY
        assert sig.parameters["temps"].default is None and sig.parameters["geo_temps"].default is None
    assert list(inspect.signature(ShardedRange.sweep).parameters) == ["self", "lonlat", "betas", "temps", "geo_temps"]
    assert {"temps", "geo_temps"} <= set(inspect.signature(ShardedRange.embed_sweep).parameters)
    assert "range_stats_kept" in _native.SYMBOLS and callable(_native.HipEngine.stats_kept)
    assert _native.PROF_KEPT_STATS == 5
    hdr = open(os.path.join(REPO, "include", "range_hip.h")).read()
    assert re.search(r"RANGE_PROF_KEPT_STATS = 5,\s*RANGE_PROF_KINDS = 6", hdr) and "#define RANGE_ABI_VERSION 9" in hdr


def test_codegen_of_the_kept_statistics_kernel():
    """Every instantiation of kept_stats_kernel (1..8 pairs x with / without a geographic head) exists,
    uses no scratch memory, no LDS allocation at all (0 bytes: no ring; the lane merge's shuffles
    allocate none) and leaves at least 4 waves per SIMD; the geographic logit is one MFMA per tile in
    flight (+ the masked last block's) and the semantic head has none.  The four pass-1 kernels keep
    their 64 / 65 MFMAs per tile."""
    from device_asm import device_asm
    out = device_asm()
    if out is None:
        pytest.skip("hipcc not available")
    kernels = {k.split(":", 1)[0]: k for k in re.split(r"\n(?=_ZN9range_hip\w+:)", open(out).read())}
    num = lambda k, pat: int(re.search(pat, k).group(1))
    mf = lambda k: len(re.findall(r"\n\s*v_mfma_f32_16x16x4_f32\b", k))
    seen = {}
    for pairs in range(1, 9):
        for geo in ("1", "0"):
            ks = [k for n, k in kernels.items() if n.startswith(f"_ZN9range_hip17kept_stats_kernelILi{pairs}ELb{geo}E")]
            assert len(ks) == 1, (pairs, geo, len(ks))
            k = ks[0]
            seen[pairs, geo] = (num(k, r"; NumVgprs: (\d+)"), num(k, r"; NumAgprs: (\d+)"), num(k, r"; Occupancy: (\d+)"))
            assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", k) and re.search(r"; ScratchSize: 0\b", k), seen
            assert num(k, r"\.amdhsa_group_segment_fixed_size (\d+)") == 0, (pairs, geo)
            assert not re.search(r"\n\s*(ds_read|ds_write|global_load_lds|s_barrier)", k), (pairs, geo)
            assert seen[pairs, geo][0] + seen[pairs, geo][1] <= 128 and seen[pairs, geo][2] >= 4, seen
            assert mf(k) == (9 if geo == "1" else 0), (pairs, geo, mf(k))      # KEPT_TILES_IN_FLIGHT + the masked block
            assert not re.search(r"\n\s*v_mfma_(?!f32_16x16x4_f32\b)", k)
    for geo in ("1", "0"):
        for name in (f"_ZN9range_hip23sharp_scan_stats_kernelILb{geo}E", f"_ZN9range_hip17scan_stats_kernelILb{geo}ELb0E",
                     f"_ZN9range_hip17scan_stats_kernelILb{geo}ELb1E"):
            ks = [k for n, k in kernels.items() if n.startswith(name)]
            assert len(ks) == 1 and mf(ks[0]) == (65 if geo == "1" else 64), (name, [mf(k) for k in ks])
    src = open(os.path.join(REPO, "range_amd", "csrc", "pass1_kept.h")).read()
    assert re.search(r"KEPT_TILES_IN_FLIGHT = 8\b", src) and re.search(r"KEPT_MAX_PAIRS = 8\b", src)


class SweepOracleShardEngine(SharpOracleShardEngine):
    """The checker engine with ``stats_kept`` from its stored e-hat: the statistics ``scan_stats`` would
    give for the kept queries, per pair with the engine's shift rule (constant up to 43, else the
    shard's largest scaled logit for both heads)."""

    def stats_kept(self, first_query, xq, taus, n_splits=0):
        assert self._kept is not None and first_query % 64 == 0 and first_query + xq.shape[0] <= self._kept.shape[0]
        assert n_splits == self.p1_splits(0)
        self.calls_kept = getattr(self, "calls_kept", 0) + 1
        e32 = self._kept[first_query:first_query + xq.shape[0]]
        kept, out = self._kept, []
        for ts, tg in taus:
            cls = SharpOracleShardEngine if max(ts, tg) > 43.0 else OracleShardEngine
            out.append(cls.scan_stats(self, e32, xq, ts, tg))
        self._kept = kept                                   # (scan_stats resets it)
        return torch.stack(out)


TEMPS, GEO_TEMPS, BETAS = (12.0, 100.0), (40.0, 200.0), (0.0, 0.5, 1.0)


def _sweep_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        N, B, L, H = 601, 130, 10, 64
        locs, vals, keys = synth.make_bank(N, 11)
        full = O.prep_bank(locs, vals, keys)
        r0, r1 = shard_rows(N, world, rank)
        shard = O.Bank(full.keys[r0:r1], full.values[r0:r1], full.xyz[r0:r1])
        w = synth.make_encoder_weights(L, H, 256, 2, 5)
        q = synth.make_queries(B, seed=100 + rank)
        e = O.encode(q, w, L)
        counts = {}

        def counting(model):
            start = model._start

            def counted(kind, src, key, *a, **kw):
                counts[key] = counts.get(key, 0) + 1
                return start(kind, src, key, *a, **kw)
            model._start = counted
            return model

        for keep in (True, False):
            eng = SweepOracleShardEngine(w, L, shard, r0)
            eng.keep_ok = keep
            model = counting(ShardedRange(eng, "RANGE+", 0.5, n_chunks=2))
            model.min_chunk = 2
            assert len(model._chunk_bounds(B)) == 2
            # the scan alone: one "reduce" (the all-gather of the statistics) per chunk
            counts.clear()
            model._scan(torch.from_numpy(q))
            scan_reduces = counts["reduce"]
            assert scan_reduces == 2
            counts.clear()
            sw = model.sweep(torch.from_numpy(q), BETAS, temps=TEMPS, geo_temps=GEO_TEMPS).numpy()
            assert sw.shape == (2, 2, 3, B, 1280)
            # ... the sweep: the scan's plus ONE per chunk for the statistics of all pairs
            assert counts["reduce"] == scan_reduces + 2, counts
            assert counts["exchange"] == 2 * (len(TEMPS) + len(GEO_TEMPS)), counts
            assert getattr(eng, "calls_kept", 0) == (2 if keep else 0)
            for i, ts in enumerate(TEMPS):
                for j, tg in enumerate(GEO_TEMPS):
                    for b, beta in enumerate(BETAS):
                        err = float(np.abs(sw[i, j, b][:, :1024] - _expect64(e, q, full, ts, tg, beta)).max())
                        assert err < 1e-5, (keep, ts, tg, beta, err)
                        assert np.array_equal(sw[i, j, b][:, 1024:], e)
            if keep:
                # embed_sweep passes the lists through (ragged steps of 64 queries per rank); the defaults of the lists
                es = model.embed_sweep(torch.from_numpy(q), BETAS, chunk=64, temps=TEMPS, geo_temps=GEO_TEMPS).numpy()
                assert es.shape == sw.shape and float(np.abs(es - sw).max()) < 1e-5
                one = model.sweep(torch.from_numpy(q), None, temps=(100.0,)).numpy()
                assert one.shape == (1, 1, 1, B, 1280)
                assert float(np.abs(one[0, 0, 0][:, :1024] - _expect64(e, q, full, 100.0, 40.0, 0.5)).max()) < 1e-5
                # both lists None: today's sweep
                plain = model.sweep(torch.from_numpy(q), (0.0, 1.0)).numpy()
                assert plain.shape == (2, B, 1280)
                assert float(np.abs(plain[1][:, :1024] - _expect64(e, q, full, 12.0, 40.0, 1.0)).max()) < 1e-5
        # RANGE: temps alone -> (T, B, 1280)
        rm = ShardedRange(SweepOracleShardEngine(w, L, shard, r0), "RANGE", None, n_chunks=2)
        rm.min_chunk = 2
        rs = rm.sweep(torch.from_numpy(q), temps=(15.0, 100.0)).numpy()
        assert rs.shape == (2, B, 1280)
        for i, ts in enumerate((15.0, 100.0)):
            assert float(np.abs(rs[i][:, :1024] - _expect64(e, q, full, ts, 0.0, 1.0)).max()) < 1e-5
        with pytest.raises(ValueError, match="RANGE\\+ only"):
            rm.sweep(torch.from_numpy(q), temps=(15.0,), geo_temps=(40.0,))
        with pytest.raises(ValueError, match="RANGE\\+ only"):
            rm.sweep(torch.from_numpy(q), (0.5,))
        ret[rank] = "ok"
    except Exception as ex:  # noqa: BLE001
        import traceback
        ret[rank] = f"{type(ex).__name__}: {ex}\n{traceback.format_exc()}"
    finally:
        dist.destroy_process_group()


def test_sharded_temperature_sweep_gloo():
    """ShardedRange.sweep(..., temps=(12, 100), geo_temps=(40, 200)) over two gloo ranks, two chunks,
    N = 601, 130 queries per rank == the float64 softmax over the WHOLE bank within 1e-5 at every grid
    point; one more statistics collective per chunk than the scan; the same without kept logits."""
    ret = mp.Manager().dict()
    mp.spawn(_sweep_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    assert dict(ret) == {r: "ok" for r in range(2)}, dict(ret)
