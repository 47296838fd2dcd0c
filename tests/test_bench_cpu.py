"""bench.py host logic on CPU: the multi-GPU launch decision (no GPU calls)."""
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
import bench  # noqa: E402


def _args(**kw):
    a = bench.parse([])
    for k_, v in kw.items():
        setattr(a, k_, v)
    return a


def test_gpus_without_launcher_spawns_ranks():
    plan = bench.launch_plan(_args(gpus=4), {}, ["--gpus", "4", "--steps", "3"])
    assert isinstance(plan, list)
    assert plan[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in plan and "--master-addr=127.0.0.1" in plan
    assert plan[-3:] == ["--gpus", "4", "--steps", "3"] or plan[-4:-1] == ["--gpus", "4", "--steps"]


def test_launcher_world_size_must_match_gpus():
    assert bench.launch_plan(_args(gpus=2), {"WORLD_SIZE": "2"}) is None
    err = bench.launch_plan(_args(gpus=8), {"WORLD_SIZE": "1"})
    assert isinstance(err, str) and "--gpus 8" in err
    # the driver's N=1 run: no launcher, no spawn
    assert bench.launch_plan(_args(gpus=1), {}) is None


def test_main_refuses_mismatched_world_size(monkeypatch):
    """A launcher with WORLD_SIZE=1 and --gpus 8: exit code 2 before any GPU call."""
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert bench.main(["--gpus", "8"]) == 2


def test_headline_workload_is_per_gpu_constant():
    """Every N runs the same generations per GPU (weak scaling); C4 is its own leg."""
    a = bench.parse([])
    assert a.G is None and a.config == "auto" and a.c4_G == 156250


def test_full_and_dump_outputs_are_off_by_default():
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_sample_mask_and_budget(tmp_path):
    """--dump-outputs on host tensors: float32 files within DUMP_MAX, the same
    seeded generations on every call, recovered rows beyond n_rec (and of a
    failed generation) written as 0 / index -1 whatever the buffer held."""
    import numpy as np
    import torch
    G, r, Lr, emax, Lb = 300, 4, 128, 4, 100
    rng = np.random.default_rng(1)
    rep = torch.from_numpy(rng.integers(0, 256, G * r * Lr, dtype=np.uint8))
    rec = torch.from_numpy(rng.integers(0, 256, G * emax * Lb, dtype=np.uint8))
    rec_index = torch.from_numpy(rng.integers(0, 64, G * emax).astype(np.int16))
    n_rec = torch.from_numpy(rng.integers(0, emax + 1, G).astype(np.int32))
    status = torch.zeros(G, dtype=torch.int32)
    status[::7] = -3
    shapes = bench.dump_outputs(torch, str(tmp_path / "a"), 0, rep, rec, rec_index, n_rec, status, G, r, Lr, emax, Lb)
    S = bench.DUMP_SAMPLE
    assert shapes == {"generations.npy": [S], "repairs.npy": [S, r, Lr], "recovered.npy": [S, emax, Lb],
                      "recovered_index.npy": [S, emax], "n_rec.npy": [G], "status.npy": [G]}
    got = {n: np.load(tmp_path / "a" / n) for n in shapes}
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_MAX
    gens = got["generations.npy"].astype(np.int64)
    assert (np.diff(gens) > 0).all() and gens.min() >= 0 and gens.max() < G
    assert (got["repairs.npy"] == rep.numpy().reshape(G, r, Lr)[gens]).all()
    assert (got["n_rec.npy"] == n_rec.numpy()).all() and (got["status.npy"] == status.numpy()).all()
    n = np.where(status.numpy() == 0, n_rec.numpy(), 0)[gens]
    valid = np.arange(emax)[None, :] < n[:, None]
    assert (got["recovered.npy"] == rec.numpy().reshape(G, emax, Lb)[gens] * valid[..., None]).all()
    assert (got["recovered_index.npy"] == np.where(valid, rec_index.numpy().reshape(G, emax)[gens], -1)).all()
    # other bytes in the undefined rows, same files
    rec2 = rec.clone().view(G, emax, Lb)
    rec2[torch.from_numpy(np.arange(emax)[None, :] >= np.where(status.numpy() == 0, n_rec.numpy(), 0)[:, None])] = 0xEE
    bench.dump_outputs(torch, str(tmp_path / "b"), 0, rep, rec2.view(-1), rec_index, n_rec, status, G, r, Lr, emax, Lb)
    for name in shapes:
        assert (np.load(tmp_path / "b" / name) == got[name]).all(), name


def test_dump_outputs_headline_and_c4_sizes_fit():
    """The byte budget at the headline's and C4's generation counts."""
    assert bench.DUMP_MAX <= 64 * 10**6
    for G, want_small in ((65536, True), (156250, True), (10_000_000, False)):
        small, S, nbytes = bench.dump_plan(G, 16, 1280, 16, 1200)
        assert small is want_small and S == bench.DUMP_SAMPLE and nbytes <= bench.DUMP_MAX
    # jumbo rows: fewer generations, still within the budget
    small, S, nbytes = bench.dump_plan(4096, 59, 9088, 59, 9000)
    assert 1 <= S < bench.DUMP_SAMPLE and nbytes <= bench.DUMP_MAX


def _recorded_full(name="r04am_bench_full.json"):
    import json
    lines = [l for l in (REPO / "profiles" / name).read_text().splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def test_line_fits_driver_parse():
    """the 20.8 KB round-4 line was not parsed by the
    driver.  The compact line of a recorded full run (every leg present) must
    stay under LINE_MAX and carry the contract keys first."""
    import json
    full = _recorded_full()
    line = bench.compact_line(full, "gpurun_out/bench_detail.json")
    s = json.dumps(line)
    assert len(s) <= bench.LINE_MAX <= 8000, len(s)
    keys = list(line)
    assert keys[:13] == ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                         "scaling", "vs_baseline", "dtype", "data", "config"]
    for k in ("roofline", "cpu_baseline", "roofline_encode", "c5", "c4", "cpu_variants_gibps"):
        assert line.get(k), k
    rl = line["roofline"]
    assert rl["bound"] == "hbm" and rl["unit"] == "GB/s" and 0 < rl["frac"] < 1
    assert abs(rl["achieved"] / rl["peak"] - rl["frac"]) < 1e-3
    cb = line["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["cores"] >= 1 and cb["value"] > 0
    assert len(line["c5"]["shapes"]) == 7
    assert json.loads(s) == line


def test_line_trims_oversized_legs():
    """Whatever a leg grows into, the line keeps the contract keys and fits."""
    import json
    full = _recorded_full()
    full["cpu_gf_mul_loop"] = {f"k{i}": {"mb_s": i} for i in range(2000)}
    full["cpu_gf_mul_loop"].update({"table": {"mb_s": 1.0}})
    full["c5"]["k32_r5"]["block/encode"]["GiBps_alg"] = "x" * 9000
    line = bench.compact_line(full)
    assert len(json.dumps(line)) <= bench.LINE_MAX
    assert line["roofline"] and line["cpu_baseline"] and line["value"] == full["value"]


def test_detail_written(tmp_path):
    import json
    full = _recorded_full()
    p = bench.emit_detail(full, str(tmp_path / "d.json"))
    assert p and json.loads(open(p).read())["value"] == full["value"]
    assert bench.emit_detail(full, "") is None


def test_cgroup_cpu_quota(tmp_path):
    """The usable-CPU count of cpu_baseline: cgroup v2 cpu.max, else v1 cfs
    quota / period, floored; None without a quota."""
    assert bench.cgroup_cpu_quota(str(tmp_path)) is None
    (tmp_path / "cpu.max").write_text("1600000 100000\n")
    assert bench.cgroup_cpu_quota(str(tmp_path)) == 16
    (tmp_path / "cpu.max").write_text("max 100000\n")
    assert bench.cgroup_cpu_quota(str(tmp_path)) is None
    (tmp_path / "cpu.max").unlink()
    (tmp_path / "cpu").mkdir()
    (tmp_path / "cpu" / "cpu.cfs_quota_us").write_text("250000")
    (tmp_path / "cpu" / "cpu.cfs_period_us").write_text("100000")
    assert bench.cgroup_cpu_quota(str(tmp_path)) == 2
    (tmp_path / "cpu" / "cpu.cfs_quota_us").write_text("-1")
    assert bench.cgroup_cpu_quota(str(tmp_path)) is None
