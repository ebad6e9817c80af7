"""Tunable retrieval temperatures, CPU side (no GPU): the validator of the Python layer, the route
function of range_amd/csrc/host_plan.h under sanitizers, the generated code of the running-max pass 1
(range_amd/csrc/pass1_sharp.h) and the sharded plumbing over gloo with a checker engine."""
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
from test_dist_cpu import LOG2E, OracleShardEngine, _free_port

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_check_temperatures():
    from range_amd.range import check_temperatures
    assert check_temperatures("RANGE", None) == (15.0, 0.0)
    assert check_temperatures("RANGE+", None, None) == (12.0, 40.0)
    for t in (0.5, 12, 43, 43.5, 1000):
        assert check_temperatures("RANGE", t) == (float(t), 0.0)
        assert check_temperatures("RANGE+", t, t) == (float(t), float(t))
        assert check_temperatures("RANGE+", None, t, "exact") == (12.0, float(t))
    for bad in (0, -1, float("nan"), float("inf"), 1000.5):
        with pytest.raises(ValueError, match="at most 1000"):
            check_temperatures("RANGE", bad)
        with pytest.raises(ValueError, match="at most 1000"):
            check_temperatures("RANGE+", bad, 40.0)
        with pytest.raises(ValueError, match="geo_temp.*at most 1000"):
            check_temperatures("RANGE+", 12.0, bad)
    with pytest.raises(ValueError, match="RANGE\\+ only"):
        check_temperatures("RANGE", 15.0, 40.0)
    with pytest.raises(ValueError, match="bf16x3"):
        check_temperatures("RANGE+", 100, None, "bf16x3")
    with pytest.raises(ValueError, match="bf16x3"):
        check_temperatures("RANGE+", 12, 100, "bf16x3")
    assert check_temperatures("RANGE+", 43, 43, "bf16x3") == (43.0, 43.0)
    with pytest.raises(ValueError, match="Unimplemented RANGE model"):
        check_temperatures("RANGE++", 12.0)


def test_load_model_refuses_bad_temperatures_before_it_loads_anything(tmp_path):
    from range_amd.load_model import load_model
    for kw in (dict(temp=0.0), dict(temp=1001.0), dict(geo_temp=float("nan"))):
        with pytest.raises(ValueError, match="at most 1000"):
            load_model("RANGE+", pretrained_path="no-such.ckpt", db_path="no-such.npz", **kw)
    with pytest.raises(ValueError, match="RANGE\\+ only"):
        load_model("RANGE", pretrained_path="no-such.ckpt", db_path="no-such.npz", geo_temp=40.0)
    with pytest.raises(ValueError, match="bf16x3"):
        load_model("RANGE+", pretrained_path="no-such.ckpt", db_path="no-such.npz", temp=100.0, pv_mode="bf16x3")
    with pytest.raises(ValueError, match="RANGE / RANGE\\+"):
        load_model("SatCLIP", pretrained_path="no-such.ckpt", temp=20.0)


def test_temperature_route_under_sanitizers(tmp_path):
    """host_plan.h: plan_temperatures - (12, 40), (43, 43) -> constant shift; (43.5, 40), (12, 200) ->
    running maximum, small batches on the two-pass route; out-of-range values refused - compiled with
    g++ under AddressSanitizer and UndefinedBehaviorSanitizer and run on the CPU."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "temp_route")
    src = os.path.join(REPO, "tests", "native", "temp_route.cpp")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "temp_route ok" in p.stdout, p.stdout + p.stderr


def test_codegen_of_the_running_max_pass1():
    """Both instantiations of sharp_scan_stats_kernel exist, use no scratch memory and fit four
    workgroups per CU like scan_stats_kernel<GEO, false>: the same (dynamic) LDS, at most 128 vector
    registers, the same MFMA count per tile."""
    from device_asm import device_asm
    out = device_asm()
    if out is None:
        pytest.skip("hipcc not available")
    kernels = {k.split(":", 1)[0]: k for k in re.split(r"\n(?=_ZN9range_hip\w+:)", open(out).read())}
    num = lambda k, pat: int(re.search(pat, k).group(1))
    seen = {}
    for geo in ("1", "0"):
        sharp = [k for n, k in kernels.items() if n.startswith(f"_ZN9range_hip23sharp_scan_stats_kernelILb{geo}E")]
        plain = [k for n, k in kernels.items() if n.startswith(f"_ZN9range_hip17scan_stats_kernelILb{geo}ELb0E")]
        assert len(sharp) == 1 and len(plain) == 1
        s, p = sharp[0], plain[0]
        regs = {name: (num(k, r"; NumVgprs: (\d+)"), num(k, r"; NumAgprs: (\d+)"), num(k, r"; Occupancy: (\d+)"))
                for name, k in (("sharp", s), ("constant", p))}
        seen[geo] = regs
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", s) and re.search(r"; ScratchSize: 0\b", s), regs
        lds = lambda k: num(k, r"\.amdhsa_group_segment_fixed_size (\d+)")
        assert lds(s) == lds(p), (lds(s), lds(p))                      # (dynamic: SCAN_LDS_BYTES at the launch, for both)
        # four workgroups of 256 threads per CU = 4 waves per SIMD: 512 / 4 = 128 registers
        assert regs["sharp"][0] + regs["sharp"][1] <= 128 and regs["sharp"][2] >= 4, f"registers (vgpr, agpr, occupancy): {regs}"
        mf = lambda k: len(re.findall(r"\n\s*v_mfma_f32_16x16x4_f32\b", k))
        assert mf(s) == mf(p) == (65 if geo == "1" else 64), (mf(s), mf(p))
    src = open(os.path.join(REPO, "range_amd", "csrc", "scan_host.h")).read()
    assert re.search(r"launch\(kernel, dim3\(\(unsigned\)p\.grid\), dim3\(256\), SCAN_LDS_BYTES", src), seen


class SharpOracleShardEngine(OracleShardEngine):
    """The checker engine with the engine's contract ABOVE 43 (range_hip.h: range_scan_stats): m is the
    largest scaled logit of the shard's rows - different on every shard."""

    def scan_stats(self, e32, xq, tau_sem, tau_geo, topk=0, keep_logits=False):
        assert not topk
        self._kept = e32.clone() if keep_logits and self.keep_ok else None
        s, g = self._logits(e32, xq)
        st = np.zeros((s.shape[0], 4), np.float64)
        for c, (z, tau) in ((0, (s, tau_sem)), (2, (g, tau_geo))):
            if tau > 0:
                t = z * tau * LOG2E
                st[:, c] = t.max(1).astype(np.float32)      # (l is relative to the m that travels: float32)
                st[:, c + 1] = np.exp2(t - st[:, c:c + 1]).sum(1)
            else:
                st[:, c] = -1e30
        return torch.from_numpy(st.astype(np.float32))


def _expect64(e, qn, bank, tau_sem, tau_geo, beta):
    s, g = O.logits64(e, qn, bank)
    V = bank.values.astype(np.float64)

    def soft(z):
        p = np.exp(z - z.max(axis=1, keepdims=True))
        return p / p.sum(axis=1, keepdims=True)
    high = soft(s * tau_sem) @ V
    return high if not tau_geo else (1 - beta) * (soft(g * tau_geo) @ V) + beta * high


def _sharp_worker(rank, world, port, ret):
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
        for name, beta, kw, taus in (("RANGE+", 0.5, dict(tau_sem=100, tau_geo=200), (100.0, 200.0)),
                                     ("RANGE+", 0.25, dict(tau_geo=200), (12.0, 200.0)),
                                     ("RANGE", None, dict(tau_sem=100), (100.0, 0.0))):
            model = ShardedRange(SharpOracleShardEngine(w, L, shard, r0), name, beta, n_chunks=2, **kw)
            model.min_chunk = 2
            assert (model.tau_sem, model.tau_geo) == taus
            out = model(torch.from_numpy(q)).numpy()
            err = float(np.abs(out[:, :1024] - _expect64(e, q, full, *taus, beta)).max())
            assert out.shape == (B, 1280) and err < 1e-5, (name, taus, err)
            assert np.array_equal(out[:, 1024:], e)
        sw = ShardedRange(SharpOracleShardEngine(w, L, shard, r0), "RANGE+", 0.5, tau_sem=100, tau_geo=200).sweep(torch.from_numpy(q), (0.0, 1.0)).numpy()
        for j, b in enumerate((0.0, 1.0)):
            assert float(np.abs(sw[j][:, :1024] - _expect64(e, q, full, 100.0, 200.0, b)).max()) < 1e-5
        # the positional signature and the defaults are what they were
        d = ShardedRange(OracleShardEngine(w, L, shard, r0), "RANGE+", 0.5, None, 1)
        assert (d.tau_sem, d.tau_geo, d.n_chunks) == (12.0, 40.0, 1)
        with pytest.raises(ValueError, match="at most 1000"):
            ShardedRange(OracleShardEngine(w, L, shard, r0), "RANGE+", 0.5, tau_sem=1001)
        with pytest.raises(ValueError, match="RANGE\\+ only"):
            ShardedRange(OracleShardEngine(w, L, shard, r0), "RANGE", None, tau_geo=40)
        ret[rank] = "ok"
    except Exception as ex:  # noqa: BLE001
        import traceback
        ret[rank] = f"{type(ex).__name__}: {ex}\n{traceback.format_exc()}"
    finally:
        dist.destroy_process_group()


def test_sharded_forward_at_sharp_temperatures_gloo():
    """ShardedRange(..., tau_sem=100, tau_geo=200) over two gloo ranks == the float64 softmax over the
    WHOLE bank: the shards' statistics carry different m (each its own largest scaled logit) and merge
    through the engine's log-sum-exp merge."""
    ret = mp.Manager().dict()
    mp.spawn(_sharp_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    assert dict(ret) == {r: "ok" for r in range(2)}, dict(ret)
