"""bench.py's output contract: ONE JSON line with the driver's keys plus `roofline`; with --full also `cpu_baseline` and the legs."""
import json
import os
import py_compile
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_bench_and_entry_compile():
    py_compile.compile(BENCH, doraise=True)
    py_compile.compile(os.path.join(ROOT, "__graft_entry__.py"), doraise=True)


def test_bench_refuses_to_run_without_a_gpu(gpu_present):
    if gpu_present:
        pytest.skip("GPU present")
    r = subprocess.run([sys.executable, BENCH, "--steps", "2", "--warmup", "1"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode != 0 and "no CPU fallback" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_bench_line_has_the_contract_keys():
    r = subprocess.run([sys.executable, BENCH, "--full", "--steps", "30", "--warmup", "5", "--preheat-ms", "50", "--cpu-seconds", "1"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 30 and d["warmup"] == 5 and d["higher_is_better"] is True
    assert d["unit"] == "Mpoints/s" and d["scaling"] == "strong" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "configs[2]" in d["config"]["workload"] and d["config"]["streams_total"] == 8 and d["config"]["ring_cold"] is True
    assert "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert rf["achieved"] > 1000                                   # sanity: > 1 TB/s on an MI355X
    # value and the per-launch figure describe the same steps
    assert abs(d["value"] - 8 * 1280 * 720 / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 0.01
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "Mpoints/s" and cb["cores"] >= 1 and cb["value"] > 0 and cb["sample"]
    assert cb["host_physical_cores"] >= 1 and cb["host_logical_cpus"] >= cb["host_physical_cores"]
    assert cb["host_logical_cpus"] == len(os.sched_getaffinity(0)) and cb["statistic"] == "median" and cb["passes"] >= 30
    # the other kernels' legs ride on the --full line, each with its own byte model
    comp = d["compaction"]
    assert 0.85 < comp["kept_fraction"] < 0.95 and abs(comp["algorithmic_bytes_per_point"] - (5 + 10 * comp["kept_fraction"])) < 1e-2
    assert comp["frac"] > 0.2 and d["batched_dense"]["frac"] > 0.3 and d["pack_twin"]["batched_frac"] > 0.2
    c5 = d["config5_one_gpu"]
    assert c5["points_in"] == 16 * 1920 * 1080 and 0.85 < c5["points_kept"] / c5["points_in"] < 0.95 and 0 < c5["voxels"] < c5["points_kept"]
    assert c5["pipeline_ms_per_frame_set"] > 0
    assert c5["one_call"]["voxels"] == c5["voxels"] and c5["one_call"]["ms_per_frame_set"] > 0
    oc = c5["one_call"]           # the frame loop over two contexts: digest-checked, and not slower than one context queueing behind itself
    assert oc["frame_loop_two_contexts_digest_ok"] is True and 0 < oc["frame_loop_two_contexts_ms_per_frame_set"] < 1.05 * oc["ms_per_frame_set"]
    assert oc["colour_row_from_table"] is True
    assert comp["batched"]["frac"] > comp["frac"]
    assert comp["caller_counts"]["frac"] > 0.2 and comp["path"].startswith("three")
    assert d["pack_twin"]["per_stream_launches_frac"] > 0.4          # round 3: the arrays are read straight into registers
    c1080 = d["color_1080p"]                                          # the real-camera geometry (depth 720p, colour 1080p, distortion)
    assert 0.2 < c1080["frac"] < d["general_rotation"]["frac"] and "1920x1080" in c1080["workload"]
    # two clocks on one region, both on the line: the event bracket (frac) and the wall clock value is computed from (frac_wall)
    assert abs(rf["frac_wall"] - rf["algorithmic_bytes_per_launch"] / (d["ms_per_step"] * 1e-3) / 1e9 / rf["peak"]) < 2e-3 and "clocks" in rf
    assert "unpinned" in d["parity"] and d["check"]["oracle_compared"]["slots"] == [0, 1]
    # BASELINE configs[1]: ONE 720p stream, device-resident, cold ring, oracle-checked, with its own roofline
    ss = d["single_stream"]
    assert "configs[1]" in ss["workload"] and ss["ring_cold"] is True and ss["check"]["oracle_compared"]["slots"] == [0, 1]
    assert ss["roofline"]["kernel"] == "pcs_fused_dense_kernel" and ss["roofline"]["algorithmic_bytes_per_launch"] == 15 * 1280 * 720
    assert abs(ss["roofline"]["frac"] - ss["roofline"]["achieved"] / 8000.0) < 1e-3 and ss["roofline"]["frac"] > 0.2
    assert ss["tile_2048_points_ms"] > 0 and ss["tile_512_points_ms"] > 0
    assert d["pack_twin"]["single"]["roofline"]["algorithmic_bytes_per_launch"] == 33 * 1280 * 720 and d["pack_twin"]["single"]["roofline"]["frac"] > 0.2
    # the drop-in where the reference lives: one camera, host pointers, beside the CPU port for ONE frame
    hs = d["host_api_single"]
    assert hs["a2_twin_ms_per_frame"]["pageable"] > 0 and hs["fused_ms_per_frame"]["pipelined_submit_collect"] > 0
    assert hs["cpu_port_ms_per_frame"]["t1"] > hs["cpu_port_ms_per_frame"]["best"] > 0 and hs["a2_twin_vs_cpu_best"] > 0
    assert "leg_errors" not in d, d.get("leg_errors")


def _bench_line(*extra, launcher=()):
    r = subprocess.run([sys.executable, *launcher, BENCH, *extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_short_and_long_runs_measure_the_same_cold_launch():
    """The driver runs --steps 20 --warmup 5. Its per-launch figure must be the one a long run (and rocprof) gives:
    one launch counter runs through pre-heat, warm-up and the timed region, so the short run cannot start on ring
    slots whose inputs still sit in the Infinity Cache (round 1's 5 % optimism)."""
    quick = ("--no-extra-legs", "--no-cpu-baseline", "--no-host-api")
    a = _bench_line("--steps", "20", "--warmup", "5", *quick)
    b = _bench_line("--steps", "400", "--warmup", "40", *quick)
    la, lb = a["roofline"]["avg_launch_ms"], b["roofline"]["avg_launch_ms"]
    # the short run must not be FASTER (that was the cache-warm optimism); it may be a little slower: its 20 launches start
    # on a GPU that idled through the barrier in front of the timed region (measured 2 % with the 23 us launch)
    assert -0.03 < (la - lb) / lb < 0.06, (la, lb)
    assert a["config"]["ring_cold"] and b["config"]["ring_cold"]


@pytest.mark.gpu
def test_two_ranks_shard_the_eight_streams():
    """N > 1 is BASELINE configs[3]'s shape: 8 streams IN TOTAL, 8/N per GPU, gathered to rank 0 in camera order.
    Control flow only (gloo, both ranks on this one GPU, host-staged gather) — the numbers mean nothing."""
    d = _bench_line("--gpus", "2", "--steps", "6", "--warmup", "2", "--preheat-ms", "20", "--debug-backend", "gloo",
                    launcher=("-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                              "--master-addr", "127.0.0.1", "--master-port", "29577"))
    assert d["n_gpus"] == 2 and d["scaling"] == "strong"
    assert d["config"]["parallelism"] == "streams sharded 4/GPU x 2" and d["config"]["streams_total"] == 8
    assert d["config"]["gather_to_rank0"] is True and "gather" in d
    assert abs(d["value"] - 8 * 1280 * 720 / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 0.01


CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "config", "roofline")


@pytest.mark.gpu
def test_plain_launch_with_two_gpus_prints_a_line_from_the_node_route():
    """`python3 bench.py --gpus 2 ...` launched PLAIN (no torch.distributed.run) on a box with one GPU: the default route at
    N > 1 is the one-process libpcs_node route; the two peers are folded onto the visible GPU (virtual peers, RCCL self
    send/recv) and the line says so. It must never exit for a launcher reason."""
    d = _bench_line("--gpus", "2", "--steps", "6", "--warmup", "2", "--preheat-ms", "20")
    for k in CONTRACT_KEYS:
        assert k in d, k
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["route"].startswith("node")
    assert d["config"]["streams_per_gpu"] == 4 and d["config"]["devices"] == [0, 0] and "virtual peers" in d["debug"] and "note" in d
    assert d["rccl_ranks"] == 1 and d["config"]["gather_to_rank0"] is True and "node_error" not in d
    assert d["check"] == {"slots": [0, 1], "streams": 8, "exchange": True}
    assert d["bytes_into_root_per_step"] == 4 * 1280 * 720 * 10 and d["points_per_stream"] == [1280 * 720] * 8
    ph = d["phases_ms"]
    assert ph["kernel"] > 0 and ph["exchange"] > 0
    assert abs(d["value"] - 8 * 1280 * 720 / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 0.01
    # the direct-store gather, measured by a child process of the same script and reported beside the RCCL figure
    ds = d["direct_store"]
    assert "error" not in ds, ds
    assert ds["ms_per_step"] > 0 and ds["checked_against_oracle"] == {"slots": [0, 1], "streams": 8, "exchange": True}
    assert d["direct_store_gather"] is False


@pytest.mark.gpu
def test_node_route_under_torchrun_lets_rank_zero_drive_the_node():
    """The driver's N > 1 command line: every rank is started, rank 0's process drives all GPUs, the others exit 0."""
    d = _bench_line("--gpus", "2", "--node-devices", "0,0", "--steps", "4", "--warmup", "1", "--preheat-ms", "10", "--mode", "drop_invalid",
                    launcher=("-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                              "--master-addr", "127.0.0.1", "--master-port", "29579"))
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 1 and d["check"]["exchange"] is True
    kept = d["points_per_stream"]
    assert len(kept) == 8 and all(0.85 * 1280 * 720 < c < 0.95 * 1280 * 720 for c in kept)
    assert d["bytes_into_root_per_step"] == 10 * sum(kept[4:])


@pytest.mark.gpu
def test_node_route_on_one_gpu_agrees_with_the_headline():
    """--route node --gpus 1 is the same kernel behind pcs_node_submit_device / pcs_node_wait. Per frame-set the node records ONE
    event on the kernel stream (what pcs_node_wait waits for): a marker packet between two 23 us kernels costs ~3 us of
    command-processor time that the headline loop, which records nothing between its launches, does not pay (measured 25.8
    vs 22.8 us). Without a communicator nothing else is queued (no hop through the communication stream)."""
    quick = ("--steps", "300", "--warmup", "40")
    a = _bench_line(*quick, "--no-extra-legs", "--no-cpu-baseline", "--no-host-api")
    b = _bench_line(*quick, "--route", "node")
    assert b["config"]["route"].startswith("node") and b["rccl_ranks"] == 0 and "configs[2]" in b["config"]["workload"]
    # (recorded: +13 .. +16 %; one box of the pool measured +18.5 %)
    assert -0.03 < (b["ms_per_step"] - a["ms_per_step"]) / a["ms_per_step"] < 0.25, (a["ms_per_step"], b["ms_per_step"])
    assert b["roofline"]["kernel"] == "pcs_fused_dense_kernel" and b["roofline"]["frac"] > 0.45


@pytest.mark.gpu
def test_node_route_config5_pipelined_matches_the_digest():
    """--workload config5 over 8 (virtual) peers = BASELINE configs[4]'s shape, 2 cameras per peer, through
    pcs_node_submit_voxel_device / pcs_node_wait_voxel; bench.py aborts unless both pipelined slots equal the oracle digest."""
    d = _bench_line("--workload", "config5", "--gpus", "8", "--node-devices", "0,0,0,0,0,0,0,0", "--steps", "4", "--warmup", "1",
                    "--preheat-ms", "10", "--ring", "2")
    assert d["n_gpus"] == 8 and "BASELINE.json configs[4]" in d["config"]["workload"] and d["config"]["streams_per_gpu"] == 2
    assert d["check"]["golden"] is True and d["rccl_ranks"] == 1
    # the 8 peers share one GPU: the line goes through the voxel sinks (nothing exchanged) and carries the exchange route beside it
    assert d["voxel_sink"] is True and d["bytes_into_root_per_step"] == 0 and d["phases_ms"]["root"] > 0
    x = d["same_gpu_peers"]["partials_exchange"]
    assert x["bytes_into_root_per_step"] > 0 and x["bytes_into_root_per_step"] % 40 == 0
    assert x["partials_reduced_per_step"] * 40 > x["bytes_into_root_per_step"] and x["phases_ms"]["root"] > 0 and x["ms_per_step"] > 0


@pytest.mark.gpu
def test_ranks_route_launched_plain_reexecutes_itself_under_torchrun():
    d = _bench_line("--gpus", "2", "--debug-backend", "gloo", "--steps", "4", "--warmup", "1", "--preheat-ms", "10")
    assert d["n_gpus"] == 2 and d["config"]["gather_to_rank0"] is True and "gloo" in d["debug"]


DUMP_FILES = ["payload_column_sums.npy", "payload_record_index.npy", "payload_records.npy"]


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_its_last_step(tmp_path, oracle):
    """A plain run sets up, warms up, times --steps launches and prints the line: no oracle check, legs, long sample or CPU sample.
    --dump-outputs writes what the last timed step computed. Pre-heat ends on a whole turn of the ring, so the last of W + K launches
    read ring slot (W + K - 1) % R, whose frame-set is host set slot % 4 (benchlegs/rig.py: DISTINCT): the dumped records are the
    oracle's records of that set, and a second run writes the same files."""
    W, K = 5, 23
    a = _bench_line("--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path / "a"))
    for k in CONTRACT_KEYS:
        assert k in a, k
    assert a["steps"] == K and a["warmup"] == W and a["dtype"] == "f32" and a["check"]["oracle_compared"] is None
    assert abs(a["value"] - 8 * 1280 * 720 / (a["ms_per_step"] * 1e-3) / 1e6) / a["value"] < 0.01
    for k in ("cpu_baseline", "speedup_vs_cpu_baseline", "compaction", "batched_dense", "config5_one_gpu", "single_stream", "host_api",
              "host_api_single", "per_kernel_unprofiled_us", "leg_errors"):
        assert k not in a, k
    assert a["roofline"]["long_sample_ms"] is None and "per_launch_ms" not in a["roofline"]
    b = _bench_line("--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path / "b"))
    assert sorted(os.listdir(tmp_path / "a")) == DUMP_FILES
    total = 0
    for f in DUMP_FILES:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
        total += os.path.getsize(tmp_path / "a" / f)
    assert total <= 64 << 20
    from pointcloud_stitching_amd import synthetic as Syn
    seed = Syn.SEED + 7919 * (((W + K - 1) % a["config"]["ring_frame_sets"]) % 4)
    cfgs = [Syn.synth_stream_config(1280, 720, s) for s in range(8)]
    dep = [Syn.synth_depth(1280, 720, s, seed=seed) for s in range(8)]
    col = [Syn.synth_color(1280, 720, s, seed=seed) for s in range(8)]
    want, _ = oracle.process_frames(cfgs, dep, col, 0, 1)
    idx = np.load(tmp_path / "a" / "payload_record_index.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "payload_records.npy"), want[idx].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "payload_column_sums.npy"), want.reshape(8, -1, 5).sum(axis=1, dtype=np.int64))


def test_dump_outputs_is_refused_where_it_cannot_be_honoured(tmp_path):
    """--full and --dump-outputs are off by default; a dump that cannot be honoured is refused before anything touches a GPU."""
    b = _load_bench_module()
    d = b.parse([])
    assert d.full is False and d.dump_outputs is None
    assert b.dump_refusal(b.parse(["--dump-outputs", "x"]), "ranks") is None
    for mode in ("batch", "pack", "pack_batch"):
        assert b.dump_refusal(b.parse(["--dump-outputs", "x", "--mode", mode]), "ranks") is None
    assert b.dump_refusal(b.parse(["--dump-outputs", "x", "--gpus", "2"]), "node")
    assert b.dump_refusal(b.parse(["--dump-outputs", "x", "--route", "node"]), "node")
    assert b.dump_refusal(b.parse(["--dump-outputs", "x", "--workload", "config5"]), "ranks")
    assert b.dump_refusal(b.parse(["--dump-outputs", "x", "--mode", "drop_invalid"]), "ranks")
    r = subprocess.run([sys.executable, BENCH, "--workload", "config5", "--dump-outputs", str(tmp_path / "d")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr and not os.path.exists(tmp_path / "d")


def test_written_outputs_are_a_fixed_sample_and_exact_sums(tmp_path):
    import torch
    from benchlegs import common as CM
    g = torch.Generator().manual_seed(3)
    for sets, per_stream in ((1, 1000), (2, 70_000)):
        pay = [torch.randint(-32768, 32768, (8 * per_stream * 5,), dtype=torch.int16, generator=g) for _ in range(sets)]
        CM.write_outputs(str(tmp_path / "a"), pay, 8)
        CM.write_outputs(str(tmp_path / "b"), pay, 8)
        assert sorted(os.listdir(tmp_path / "a")) == DUMP_FILES
        recs = torch.cat(pay).view(-1, 5).numpy()
        rec, idx = np.load(tmp_path / "a" / "payload_records.npy"), np.load(tmp_path / "a" / "payload_record_index.npy")
        assert rec.dtype == np.float32 and idx.dtype == np.float64
        assert len(idx) == min(recs.shape[0], CM.DUMP_RECORDS) and np.all(np.diff(idx) > 0)
        assert np.array_equal(rec, recs[idx.astype(np.int64)].astype(np.float32))
        sums = np.load(tmp_path / "a" / "payload_column_sums.npy")
        assert sums.shape == (sets * 8, 5) and np.array_equal(sums, recs.reshape(sets * 8, -1, 5).sum(axis=1, dtype=np.int64))
        for f in DUMP_FILES:
            assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def _load_bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_leg_guard_records_and_swallows_exceptions():
    """A failing leg must not cost the line: the exception is recorded under leg_errors and the run goes on."""
    b = _load_bench_module()
    out = {}
    with b.Leg(out, "broken"):
        raise RuntimeError("boom")
    with b.Leg(out, "fine"):
        out["fine"] = 1
    assert out["fine"] == 1 and "RuntimeError: boom" in out["leg_errors"]["broken"] and "fine" not in out["leg_errors"]
    with pytest.raises(KeyboardInterrupt):          # not an Exception: must propagate
        with b.Leg(out, "interrupted"):
            raise KeyboardInterrupt


def test_a_swallowed_leg_is_named_on_the_line():
    """Every leg of the line is a function (benchlegs/legs_*.py) run through run_leg: what it returns lands under its name, a leg
    that does not apply (returns None) leaves nothing, and a leg that raises is NAMED under leg_errors — silently missing is not an
    outcome. The legs bench.py wires are importable without a GPU, and each is a plain function of the rig."""
    b = _load_bench_module()
    out = {"roofline": {}}

    def good(x, y=1):
        return {"sum": x + y}

    def broken():
        raise ValueError("no such ring slot")
    assert b.run_leg(out, "good", good, 2, y=3) == {"sum": 5} and out["good"] == {"sum": 5}
    assert b.run_leg(out, "not_applicable", lambda: None) is None and "not_applicable" not in out
    assert b.run_leg(out, "broken", broken) is None and "broken" not in out
    assert out["leg_errors"] == {"broken": "ValueError: no such ring slot"}
    b.run_leg(out, "per_launch_ms", lambda: {"n": 3}, into=out["roofline"])          # a leg may report into another leg's object
    assert out["roofline"]["per_launch_ms"] == {"n": 3} and "per_launch_ms" not in out
    import inspect
    from benchlegs import legs_dense, legs_config5, legs_host, legs_single
    src = open(BENCH).read()
    for mod, names in ((legs_dense, ("compaction", "batched_dense", "pack_twin", "centre_transform", "infinity_cache_resident_inputs",
                                     "two_stream_overlap", "general_rotation", "color_1080p", "per_launch_ms")),
                       (legs_config5, ("config5_one_gpu",)), (legs_host, ("host_api", "host_api_single")), (legs_single, ("single_stream",))):
        for n in names:
            fn = getattr(mod, n)
            assert inspect.isfunction(fn) and list(inspect.signature(fn).parameters)[0] == "g"
            assert f'run_leg(out, "{n}"' in src, n            # wired under its own name: that is the name leg_errors would show
    assert "with Leg(" not in src                            # no leg body lives in bench.py any more


def test_cpu_sample_reports_physical_cores():
    from oracle import cpu_baseline as CB
    n = CB._physical_cores()
    assert n is None or (1 <= n <= (os.cpu_count() or 1))
    allowed = os.sched_getaffinity(0)
    m = CB._physical_cores(allowed)
    assert m is None or (1 <= m <= len(allowed))


def test_cpu_sample_child_process_line():
    """bench.py's cpu_baseline leg runs oracle/cpu_baseline.py as a child with the OpenMP team bound; the object it prints
    carries the median, its spread and where the team ran. (A tiny geometry: this is the contract, not a measurement.)"""
    b = _load_bench_module()
    d = b.cpu_baseline(64, 48, 2, 0.3)
    assert d["kind"] == "port" and d["unit"] == "Mpoints/s" and d["statistic"] == "median" and d["passes"] >= 30
    assert d["p10_value"] <= d["value"] <= d["p90_value"] <= d["best_value"]
    assert d["cores"] >= 1 and len(d["team_cpus"]) == d["cores"] and d["t1_value"] > 0 and d["with_deprojection_value"] > 0
    assert "OMP_PROC_BIND=close" in d["sample"] and "OMP_PLACES=cores" in d["sample"]
    assert d["host_physical_cores"] >= 1 and d["host_logical_cpus"] >= d["host_physical_cores"]
    # the child reads its CPU set before libgomp binds the master thread to the first place
    assert d["host_logical_cpus"] == len(os.sched_getaffinity(0))


def test_route_choice_never_depends_on_how_the_script_was_launched():
    """`--gpus N` must produce a line however it is started (round-3 verdict: a plain launch exited). The decision table:"""
    b = _load_bench_module()
    many, one = (lambda: 8), (lambda: 1)
    # N = 1: the single-GPU legs; N > 1 plain: the one-process node route; under torch.distributed.run: the same (rank 0 drives it)
    assert b.choose_route("auto", 1, "", "nccl", 1, {}, many) == "ranks"
    assert b.choose_route("auto", 8, "", "nccl", 1, {}, many) == "node"
    assert b.choose_route("auto", 8, "", "nccl", 8, {}, many) == "node"
    # fewer GPUs than asked for, nothing hidden: still the node route (it folds the peers and says so)
    assert b.choose_route("auto", 8, "", "nccl", 8, {}, one) == "node"
    assert b.choose_route("auto", 2, "", "nccl", 1, {}, one) == "node"
    # a launcher that shows every rank only its own GPU: rank 0 cannot drive the others -> one process per GPU
    assert b.choose_route("auto", 8, "", "nccl", 8, {"HIP_VISIBLE_DEVICES": "3"}, one) == "ranks"
    assert b.choose_route("auto", 8, "", "nccl", 8, {"ROCR_VISIBLE_DEVICES": "0,1,2,3,4,5,6,7"}, many) == "node"
    # explicit peers (virtual peers), the gloo control-flow test, explicit routes
    assert b.choose_route("auto", 2, "0,0", "nccl", 2, {"HIP_VISIBLE_DEVICES": "0"}, one) == "node"
    assert b.choose_route("auto", 2, "", "gloo", 1, {}, one) == "ranks"
    assert b.choose_route("ranks", 8, "", "nccl", 1, {}, many) == "ranks" and b.choose_route("node", 1, "", "nccl", 1, {}, one) == "node"


def test_readme_quotes_only_the_recorded_bench_line():
    """README.md's results table is generated from ONE recorded `python bench.py` line (profiles/r06_bench.json) by
    tools/readme_results.py; regenerating it must give the text README holds, and no other 'Mpoints/s' figure may stand in
    README outside that block (round 4 had four different GPU/CPU ratios in four documents)."""
    import importlib.util
    import re
    spec = importlib.util.spec_from_file_location("readme_results", os.path.join(ROOT, "tools", "readme_results.py"))
    rr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rr)
    src = os.path.join("profiles", "r06_bench.json")
    want = rr.table(rr.load(os.path.join(ROOT, src)), src)
    readme = open(os.path.join(ROOT, "README.md")).read()
    a, b = readme.index(rr.BEGIN), readme.index(rr.END) + len(rr.END)
    assert readme[a:b] == want, "README's results block is stale: python tools/readme_results.py --write"
    outside = readme[:a] + readme[b:]
    assert not re.search(r"\d\s*k?\s*Mpoints/s", outside), "a throughput figure outside the generated block"
    assert not re.search(r"GPU\s*=\s*\d+", outside)
    d = rr.load(os.path.join(ROOT, src))
    assert d["n_gpus"] == 1 and "configs[2]" in d["config"]["workload"] and "leg_errors" not in d
    # the block carries the parity sentence of the line itself: bit-exact against this build's own restatement, unpinned
    assert "unpinned" in d["parity"] and ("Parity: " + d["parity"]) in readme[a:b]


def test_the_line_is_the_last_line_on_stdout_even_after_c_level_prints():
    """RCCL prints its version banner with printf; through a pipe the C buffer is flushed at exit — after anything Python printed —
    unless bench.py flushes it first. A child process: printf through libc, then bench.emit; the pipe must end with the JSON line."""
    code = ("import ctypes, importlib.util, sys\n"
            "ctypes.CDLL(None).printf(b'RCCL version : banner from C stdio\\n')\n"
            f"spec = importlib.util.spec_from_file_location('bench_module', {BENCH!r})\n"
            "b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)\n"
            "b.emit({'metric': 'm', 'value': 1.0})\n")
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert lines[0].startswith("RCCL version") and json.loads(lines[-1]) == {"metric": "m", "value": 1.0}
