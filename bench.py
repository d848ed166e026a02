#!/usr/bin/env python3
"""bench.py -- one controller cycle of kompass_cpp's sampling-controller hot path
(BASELINE.json configs[1]: DWA diff-drive, 8192 samples x 50 steps, 500x500
costmap) on N MI355X, through the C ABI of libkompass_hip.so.

A "step" is one full cycle over one batch of synthetic input: host trig table
(BAR stores), roll-out + collision gate + path / obstacle costs + ordered cost
finalisation + argmin + result record in ONE kernel launch (kc_dwa_cycle;
`--split`: the three-kernel cycle), [N>1: one 8-byte RCCL all-reduce(min)],
result to the host.  Sensor data, tracked segment and the sample lattice are
resident in HBM before the timed region starts.

The headline line is BASELINE configs[1] on SURVEY 8(d)'s scene (Bernoulli 0.02
clutter: only ~5 % of the samples survive the collision gate, so the cost stage
has little to do -- `config.workload` says how many).

A plain run does only what the headline needs: set-up, warm-up, the timed steps,
--dump-outputs, one JSON line.  `--full` adds everything else the line measures
and checks: per-kernel HIP-event times and the roofline (a second pass over the
steps), the CPU baseline with its winner check, and the legs beside the headline
-- the cycle on two more scenes of the same lattice (`mid_density`: about half
admissible, `open_space`: every sample admissible), LaserScan input, the input
updates, fresh inputs every cycle, the cfg4 mapper; with several ranks the
strong-scaling block.

Contract: `python bench.py --gpus N --steps K --warmup W`.  For N > 1 the ranks are one
process per GPU: either the caller starts them (`python -m torch.distributed.run --nnodes=1
--nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...`), or -- no
WORLD_SIZE in the environment -- this script starts them itself, as child processes, BEFORE it
touches the GPU (a process that has initialised HIP must never be replaced or forked into ranks),
relays rank 0's line and exits with the launcher's return code.  Rank 0 prints ONE JSON line.

With fewer GPUs than ranks (rehearsal on a one-GPU box) the ranks share the devices and exchange
through the library's shared-memory transport instead of RCCL (which refuses two ranks on one
device); `config.collective` says which transport ran.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

# numpy's BLAS starts one thread per hardware thread it sees (256 on the GPU box, whose
# container may use 16): that burst alone gets the process CPU-throttled for a period or two.
# Nothing here needs a threaded BLAS.
for _v in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "4")
# dmabuf IPC: RCCL between rank processes on this pool fails with the legacy mode (hipIpcGetMemHandle).
# Set here -- before torch or libkompass_hip.so is imported, i.e. before anything touches the GPU -- so that
# ranks started by an EXTERNAL launcher (python -m torch.distributed.run ... bench.py --gpus N) have it too,
# not only the children of launch_ranks().
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402

ROOT = Path(__file__).resolve().parent
for p in (ROOT, ROOT / "kompass-core_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def pmc_traffic(kernel, scene="survey", cfg="cfg2"):
    """HBM bytes per launch of `kernel` from the newest committed PMC pass of that config and scene
    (profiles/*_<cfg>_<scene>_pmc_hbm.json: separate FETCH_SIZE / WRITE_SIZE runs of this same
    command, gfx950 correction applied); (None, None) when no pass of this workload is committed."""
    import glob
    import json as _json

    files = sorted(glob.glob(str(ROOT / "profiles" / f"*_{cfg}_{scene}_pmc_hbm.json")))
    if not files:
        return None, None
    rec = _json.load(open(files[-1])).get("kernels", {}).get(kernel)
    if not rec:
        return None, None
    return rec.get("hbm_bytes_per_launch_corrected"), os.path.basename(files[-1])


GPU_SIMDS, GPU_CLOCK_HZ = 1024, 2.4e9  # MI355X_MICROARCH.md: 256 CUs x 4 SIMDs, 2.4 GHz


def profile_kernel_ms(stats_csv, kernel):
    """Average duration (ms) of `kernel` in a committed rocprofv3 --stats summary, or None."""
    import csv

    short = {"cycle_kernel": "rollout_collide_kernel<32, 1024, kc::CycleTail>"}.get(kernel, kernel)
    try:
        with open(stats_csv) as f:
            for row in csv.DictReader(f):
                if short in row["Name"]:
                    return float(row["AverageNs"]) * 1e-6
    except (OSError, KeyError, ValueError):
        pass
    return None


def pmc_explain(kernel, scene, cfg, launch_ms):
    """What binds the kernel when HBM does not ('VALU utilisation + launch count as the explanatory
    figures'), from the newest committed SQ counter passes of this workload (profiles/*_<cfg>_<scene>_pmc_sq.json:
    separate rocprofv3 --pmc passes, means per launch summed over the chip) and the phase clocks of the kernel
    (profiles/*_<cfg>_<scene>_phase_stamps.json: s_memrealtime stamps of a -DKC_PHASE_STAMPS build)."""
    import glob
    import json as _json

    out = {}
    files = sorted(glob.glob(str(ROOT / "profiles" / f"*_{cfg}_{scene}_pmc_sq.json")))
    rec = _json.load(open(files[-1])).get("kernels", {}).get(kernel) if files else None
    if rec and rec.get("SQ_ACTIVE_INST_VALU"):
        # Counter and duration from the SAME collection (one box): the kernel's average in the
        # *_kernel_stats.csv that was written beside the counter file.  (Round 3 divided the committed counter by
        # THIS run's launch time -- two different boxes of a pool that differ by 10 %.)
        prof_ms = profile_kernel_ms(files[-1].replace("_pmc_sq.json", "_kernel_stats.csv"), kernel)
        if prof_ms:
            # SQ_ACTIVE_INST_VALU counts quad-cycles in which a SIMD issues VALU work: x 4 = SIMD cycles, over the
            # SIMD cycles the launch lasted on the whole chip
            out["valu_issue_frac"] = rec["SQ_ACTIVE_INST_VALU"] * 4.0 / (GPU_SIMDS * GPU_CLOCK_HZ * prof_ms * 1e-3)
            out["valu_issue_frac_launch_ms"] = prof_ms
        if rec.get("SQ_INSTS_SALU") and rec.get("SQ_INSTS_VALU"):
            out["salu_per_valu"] = rec["SQ_INSTS_SALU"] / rec["SQ_INSTS_VALU"]
        if rec.get("SQ_LDS_BANK_CONFLICT") is not None and rec.get("SQ_ACTIVE_INST_LDS"):
            out["lds_conflict_frac"] = rec["SQ_LDS_BANK_CONFLICT"] / (4.0 * rec["SQ_ACTIVE_INST_LDS"])
        if rec.get("SQ_INSTS_VALU") and rec.get("SQ_WAVES"):
            out["valu_insts_per_wave"] = rec["SQ_INSTS_VALU"] / rec["SQ_WAVES"]
        out["counters_source"] = os.path.basename(files[-1])
        out["counters_box"] = ("the box of the committed profile (counters and the launch time they are divided by come from "
                               "the same collection); avg_launch_ms / achieved / frac above are THIS run's")
    files = sorted(glob.glob(str(ROOT / "profiles" / f"*_{cfg}_{scene}_phase_stamps.json")))
    if files:
        st = _json.load(open(files[-1]))
        if st.get("kernel") == kernel:
            out["critical_path_us"] = st.get("phases_us")
            out["critical_path_source"] = os.path.basename(files[-1])
    return out


DUMP_LIMIT_BYTES = 64 << 20


def cycle_outputs(ctx, r, ranks=None):
    """What a caller of the controller cycle receives: the result record (float64; the cost stays float32) and,
    when a trajectory was found, the winner's path and velocity profile (kc_dwa_get_best).  With ranks, the
    rank that owns the winner supplies the path (a collective: every rank calls this)."""
    out = {k: np.asarray(getattr(r, k), np.float32 if k == "cost" else np.float64) for k, _ in r._fields_}
    best = None
    if r.found and (ranks is None or ctx.owns_sample(r.raw_index)):
        px, py, (bvx, bvy, bom) = ctx.get_best()
        best = {"best_path_x": px, "best_path_y": py, "best_vx": bvx, "best_vy": bvy, "best_omega": bom}
    if ranks is not None:
        best = next((b for b in ranks.gather(best) if b is not None), None)
    out.update(best or {})
    return out


def write_outputs(dirname, arrays):
    """--dump-outputs: one DIR/<name>.npy per array, float32 / float64, at most DUMP_LIMIT_BYTES in all."""
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    d = Path(dirname)
    d.mkdir(parents=True, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(d / f"{name}.npy", a)


def algorithmic_bytes(N, P, map_side, S, O):
    """16 B per trajectory-step (8 B x,y written by the
    roll-out + 8 B read back by the cost pass) + 20 B per sample (12 B velocity
    in, 4 B cost out, 4 B admissible flag) + per-cycle constants (bit-packed
    costmap, tracked segment, obstacle list)."""
    return 16 * N * P + 20 * N + map_side * map_side // 8 + 12 * S + 8 * O


class Ranks:
    """torch.distributed as the control plane of a multi-rank run (rendezvous, barriers, max over
    ranks of the timing contract) -- the data path is the library's own collective.  `rehearsal`:
    more ranks than GPUs, the ranks share devices (gloo barriers, shared-memory exchange)."""

    def __init__(self, rank, world, local_rank):
        import torch
        import torch.distributed as dist

        self.torch, self.dist = torch, dist
        self.rank, self.world = rank, world
        ndev = torch.cuda.device_count()  # (does not initialise the GPU)
        if ndev < 1:
            raise SystemExit("bench.py needs a HIP device; none visible (no CPU fallback)")
        self.rehearsal = world > ndev
        self.device = local_rank % ndev
        if world == 1:  # forced (KC_BENCH_FORCE_DIST=1): no launcher has set the rendezvous up
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29517")
        torch.cuda.set_device(self.device)
        # gloo for the control plane on every run: the ONLY RCCL communicator of a rank is the one inside
        # libkompass_hip.so that carries the cycle's all-reduce (no second communicator beside it)
        dist.init_process_group("gloo", rank=rank, world_size=world)

    def barrier(self):
        self.dist.barrier()
        self.torch.cuda.synchronize()

    def max(self, *vals):
        t = self.torch.tensor(list(vals), dtype=self.torch.float64, device="cpu")
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return [float(v) for v in t.tolist()]

    def gather(self, obj):
        out = [None] * self.world
        self.dist.all_gather_object(out, obj)
        return out

    def comm(self, kh):
        """The library's communicator: RCCL (unique id from rank 0), or the shared-memory rehearsal transport."""
        if self.rehearsal:
            import uuid

            if self.torch.cuda.device_count() >= self.world:  # (cannot happen: rehearsal means fewer GPUs than ranks)
                raise SystemExit("the shared-memory transport is a rehearsal for boxes with fewer GPUs than ranks; "
                                 "with a GPU per rank the exchange goes through RCCL")

            name = [uuid.uuid4().hex[:16] if self.rank == 0 else None]
            self.dist.broadcast_object_list(name, src=0)
            return kh.Comm(self.rank, self.world, device=self.device, shm_name=name[0])
        ids = [kh.comm_unique_id() if self.rank == 0 else None]
        self.dist.broadcast_object_list(ids, src=0)
        return kh.Comm(self.rank, self.world, ids[0], device=self.device)

    def close(self):
        self.dist.barrier()
        self.dist.destroy_process_group()


def controller_bench(args, rank, world, local_rank):
    # KC_BENCH_FORCE_DIST=1 exercises the multi-GPU code path (the exchange record through a real
    # ncclAllReduce) with a single rank, e.g. on a one-GPU box
    use_dist = world > 1 or os.environ.get("KC_BENCH_FORCE_DIST") == "1"
    ranks = Ranks(rank, world, local_rank) if use_dist else None
    import kompass_hip as kh
    import sharding
    import synthetic as syn

    if kh.device_count() < 1:
        raise SystemExit("bench.py needs a HIP device; none visible (no CPU fallback)")
    device = ranks.device if ranks else local_rank

    cfg = args.config
    base = syn.CONFIGS[cfg]
    # weak scaling: every rank owns one BASELINE-sized block of the lattice
    inp = syn.make_controller_inputs(cfg, seed=0, scene=args.scene)
    n_vx, n_om = base["n_vx"], base["n_om"]
    if base["ctr"] == syn.OMNI:
        vx, vy, om = syn.lattice_omni(n_vx * world, base["n_vy"], n_om)
    else:
        vx, vy, om = syn.lattice_nonholonomic(n_vx * world, n_om)
    n_total = len(vx)
    first, count = sharding.shard_range(n_total, rank, world)
    P, S, O = inp["P"], len(inp["seg_xyz"]), len(inp["points"])

    cl, ca = CLASS_SAMPLES[cfg]
    cap = n_total if use_dist else min(65536, max(n_total, (cl + 2) * (ca + 2)))  # (the fresh_inputs leg draws a class-level window)
    ctx = kh.DwaContext(inp["robot"]["shape"], inp["robot"]["dims"], (0, 0, 0), (0, 0, 0, 1),
                        inp["octree_res"], inp["dt"], max_samples=cap, max_points=P,
                        max_segment=S, max_obstacles=O, acc_limits=inp["acc_limits"], device=device)
    if args.split:
        ctx.set_option("fused_cycle", 0)
    ctx.set_weights(kh.make_weights(*inp["weights"]))
    ctx.set_points(inp["state"], inp["points"], inp["max_range"])
    ctx.set_tracked_segment(inp["seg_xyz"], inp["acc_at_seg"], inp["ref_len"])
    # weak scaling: rank r's share is the r-th BASELINE-sized block of the (vx-major) lattice
    # (kc_dwa_set_shard_rule: every rank is handed the full list and keeps its share)
    if use_dist:
        ctx.set_shard_rule(rank, world, kh.SHARD_BLOCKS)
    ctx.set_samples(vx, vy, om)

    # data path: the library's own communicator (kc_comm_*: no framework between the kernels and
    # the collective, everything on the context's stream); torch.distributed only carries the
    # 128-byte unique id and the barriers / max-over-ranks of the timing contract
    comm = ranks.comm(kh) if use_dist else None

    def pose(i):  # a new pose every cycle: nothing can be reused between steps
        return (0.0, 0.0, 1e-3 * ((i % 7) - 3), 0.0)

    def one_cycle(i):
        if not use_dist:
            return ctx.cycle(pose(i), P)  # the whole cycle in one ABI call (one launch)
        # this rank's share + ONE all-reduce(min) of the exchange record (best key, error word, every rank's
        # admissible bitmap) + hand-off: one ABI call, the same result on every rank
        return ctx.cycle_sharded(comm, pose(i), P)

    def barrier():
        if use_dist:
            ranks.barrier()

    if args.scan and not use_dist:  # profiling passes of the laserscan_room leg: that leg alone, as the top-level line
        leg = laserscan_leg(ctx, cfg, inp, vx, vy, om, P, S, pose, args)
        leg.update({"n_gpus": 1, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                    "dtype": "f64 roll-out / f32 costs", "data": "synthetic"})
        ctx.close()
        return leg
    if args.fresh and not use_dist:
        leg = fresh_inputs_leg(kh, syn, ctx, cfg, inp, pose, args)
        leg.update({"n_gpus": 1, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                    "dtype": "f64 roll-out / f32 costs", "data": "synthetic"})
        ctx.close()
        return leg
    for i in range(args.warmup):
        one_cycle(i)
    # ---- timed region: EXACTLY args.steps cycles, barrier + sync on both sides
    lat = []
    barrier()
    t0 = time.perf_counter()
    last = None
    for i in range(args.steps):
        ts = time.perf_counter()
        last = one_cycle(i)
        lat.append(time.perf_counter() - ts)
    barrier()
    elapsed = time.perf_counter() - t0
    if use_dist:
        elapsed = ranks.max(elapsed)[0]
    if args.dump_outputs:  # the last timed cycle's outputs, before anything else runs on the context
        dumped = cycle_outputs(ctx, last, ranks)
        if rank == 0:
            write_outputs(args.dump_outputs, dumped)
    kernel_ms, host_ms = {}, {}
    if args.full:
        # ---- same cycles again with HIP events around every kernel, recorded on the
        # stream the kernels are launched on (roofline leg; events cost a few us per
        # cycle, so they stay out of `value`)
        ctx.timing_enable(True)
        for i in range(args.steps):
            one_cycle(i)
            for name, ms in ctx.timings():
                (host_ms if name.startswith("host:") else kernel_ms).setdefault(name, []).append(ms)
        ctx.timing_enable(False)
        last = one_cycle(args.steps - 1)

    # ---- result of the last cycle, pose(args.steps - 1) (for the parity check below) ----
    found, cost, raw = bool(last.found), float(last.cost), int(last.raw_index)
    if use_dist:
        # what the transport itself reports: ncclCommCount / ncclCommUserRank / ncclCommCuDevice (kc_comm_query)
        q_n, q_rank, q_dev = comm.query()
    seen = ranks.gather({"rank": rank, "device": device, "pid": os.getpid(), "comm_world": comm.world,
                         "transport": comm.transport, "comm_count": q_n, "comm_user_rank": q_rank, "comm_device": q_dev,
                         "winner": [found, cost, raw, int(last.index)]}) if use_dist else None

    out = None
    if rank == 0:
        ms_per_step = 1e3 * elapsed / args.steps
        steps_total = n_total * P  # trajectory-steps per cycle over all ranks
        value = steps_total * args.steps / elapsed
        # (the same pose as the cpu_baseline's winner and count: the last timed cycle)
        n_adm = int(last.n_admissible) if not use_dist else None
        n_adm_global = int(last.n_admissible) if use_dist else n_adm
        robot = 'omni' if base['ctr'] == 2 else 'diff-drive' if base['ctr'] == 1 else 'Ackermann'
        out = {
            "metric": "trajectory-steps/s", "value": value, "unit": "trajectory-steps/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64 roll-out / f32 costs", "data": "synthetic",
            "config": {
                "workload": f"{cfg}: DWA {robot}, {count} samples x {P} steps per GPU, "
                            f"{base['map_side']}x{base['map_side']}@0.05 costmap, scene '{args.scene}' "
                            f"({O} occupied cells; {n_adm if n_adm is not None else 'n/a'} of {count} samples "
                            f"admissible after the collision gate), tracked segment {S} pts, weights "
                            f"path/goal/obstacles; every one of the {count} x {P} steps is rolled out and "
                            f"collision-checked, costs are computed for the admissible samples",
                "scene": args.scene, "n_admissible": n_adm, "n_admissible_all_ranks": n_adm_global,
                "samples_per_gpu": count, "global_samples": n_total, "points": P,
                "parallelism": f"sample-shard x{world}" if world > 1 else "single GPU",
                "trig": ("device: the roll-out kernel evaluates glibc's sincos algorithm itself, bit-equal to the host libm "
                         "(csrc/kc_trig_exact.h); no host table, no host threads in the cycle"
                         if ctx.get_option("device_trig") else "host libm table over the BAR (KC_DEVICE_TRIG=0)"),
            },
            "latency_p50_ms": float(np.percentile(np.array(lat) * 1e3, 50)),
            "latency_min_ms": float(np.min(lat) * 1e3), "latency_max_ms": float(np.max(lat) * 1e3),
            "winner": {"found": found, "cost": cost, "raw_index": raw},
        }
        if args.full:
            out["config"]["launches_per_cycle"] = len(kernel_ms)
            out["config"]["cycle"] = (
                "single launch (kc_dwa_cycle)" if "cycle_kernel" in kernel_ms else
                "three kernels" + (" (--split)" if args.split else " (kc_dwa_cycle keeps them beyond one resident "
                                   "wave of workgroups and for small shards with many survivors)"))
            out["kernels_ms"] = {k: float(np.mean(v)) for k, v in kernel_ms.items()}
            out["host_phases_ms"] = {k: float(np.mean(v)) for k, v in host_ms.items()}
            out["roofline"] = roofline_of(kernel_ms, count, P, base["map_side"], S, O, args.scene, cfg)
        if world == 1 and args.full and not args.no_cpu:
            out["cpu_baseline"] = cpu_baseline(inp, vx, vy, om, pose(args.steps - 1), found, cost, raw, args,
                                               args.cpu_seconds)
        if use_dist:
            rw = sharding.words_per_rank([count])
            out["config"]["collective"] = (
                f"kc_dwa_cycle_sharded: ONE all-reduce(int64 x {2 + world * rw}, min) per cycle -- best key, error word, "
                f"every rank's admissible bitmap ({rw} words per rank) -- " +
                ("RCCL inside libkompass_hip.so" if comm.transport == "rccl" else
                 "REHEARSAL: the ranks share GPUs, host shared-memory transport instead of RCCL"))
            out["config"]["transport"] = comm.transport
            out["n_ranks_seen"] = int(q_n)  # ncclCommCount of the library's communicator (shm: ranks attached)
            out["n_ranks_seen_source"] = "ncclCommCount" if comm.transport == "rccl" else "shm segment attach count"
            if any(s_["comm_count"] != world or s_["comm_user_rank"] != s_["rank"] for s_ in seen):
                raise SystemExit(f"the communicator disagrees with the launcher: {seen}")
            out["ranks"] = seen
            out["ranks_agree"] = all(s_["winner"] == seen[0]["winner"] for s_ in seen)
            out["winner"]["index"] = int(last.index)
        if world == 1 and not use_dist and args.full and not args.only_headline:
            # the same lattice on the two other scenes: each a bench line of its own
            for key, scene in (("mid_density", "mid"), ("open_space", "open")):
                if scene == args.scene:
                    continue
                out[key] = scene_leg(ctx, cfg, scene, inp, vx, vy, om, P, S, pose, args)
            out["laserscan_room"] = laserscan_leg(ctx, cfg, inp, vx, vy, om, P, S, pose, args)
            ctx.set_points(inp["state"], inp["points"], inp["max_range"])
            out["extras"] = extras(ctx, inp, P, pose)
            # one REFERENCE cycle per step: fresh sensor data, window + lattice, tracked segment, cycle
            out["fresh_inputs"] = fresh_inputs_leg(kh, syn, ctx, cfg, inp, pose, args)
            # ... which is the figure a robot pays (dwa.h:183-230: new sensor data every cycle): beside the headline
            # at the top level, so that a record that keeps only the top-level fields keeps it
            out["fresh_ms_per_step"] = out["fresh_inputs"]["ms_per_step"]
            out["fresh_latency_p50_ms"] = out["fresh_inputs"]["latency_p50_ms"]
            out["fresh_value"] = out["fresh_inputs"]["value"]
            # BASELINE configs[3] in the same record: 4096-beam scan -> 1000 x 1000 grid
            margs = argparse.Namespace(**vars(args))
            margs.steps, margs.warmup = min(args.steps, 500), min(args.warmup, 50)
            out["mapper_cfg4"] = mapper_bench(margs)
    if use_dist and args.full and not args.only_headline:
        strong = {}
        for scfg in ("cfg3", "cfg5"):
            leg = strong_leg(kh, syn, sharding, scfg, rank, world, device, comm, args, ranks)
            if rank == 0:
                strong[scfg] = leg
        if rank == 0:
            out["strong"] = strong
    if use_dist:
        ranks.barrier()
        comm.close()
        ranks.close()
    ctx.close()
    return out


def strong_leg(kh, syn, sharding, cfg, rank, world, device, comm, args, ranks):
    """BASELINE configs[2] / configs[4] as they are named: ONE fixed batch (32768 / 65536 samples)
    split over the N GPUs -- strong scaling; per N the p50 cycle latency and the whole-job rate.
    Shares dealt by trig row (KC_SHARD_ROWS): a rank evaluates 1 / N of the host's cos / sin table.
    Scene 'mid' (about half of the samples admissible: SURVEY 8d's scene leaves cfg3 none)."""
    inp = syn.make_controller_inputs(cfg, seed=0, scene="mid")
    n_total, P = len(inp["vx"]), inp["P"]
    ctx = kh.DwaContext(inp["robot"]["shape"], inp["robot"]["dims"], (0, 0, 0), (0, 0, 0, 1), inp["octree_res"],
                        inp["dt"], max_samples=n_total, max_points=P, max_segment=len(inp["seg_xyz"]),
                        max_obstacles=len(inp["points"]), acc_limits=inp["acc_limits"], device=device)
    ctx.set_weights(kh.make_weights(*inp["weights"]))
    ctx.set_points(inp["state"], inp["points"], inp["max_range"])
    ctx.set_tracked_segment(inp["seg_xyz"], inp["acc_at_seg"], inp["ref_len"])
    ctx.set_shard_rule(rank, world, kh.SHARD_ROWS)
    ctx.set_samples(inp["vx"], inp["vy"], inp["omega"])
    count, trig_rows = int(ctx.get_option("shard_samples")), int(ctx.get_option("trig_rows"))
    pose = lambda i: (0.0, 0.0, 1e-3 * ((i % 7) - 3), 0.0)
    steps, warm = max(50, args.steps // 4), max(10, args.warmup // 4)
    for i in range(warm):
        ctx.cycle_sharded(comm, pose(i), P)
    lat = []
    ranks.barrier()
    t0 = time.perf_counter()
    for i in range(steps):
        ts = time.perf_counter()
        r = ctx.cycle_sharded(comm, pose(i), P)
        lat.append(time.perf_counter() - ts)
    ranks.barrier()
    el = time.perf_counter() - t0
    el, p50 = ranks.max(el, float(np.percentile(np.array(lat) * 1e3, 50)))
    single = int(ctx.get_option("last_cycle_single_launch"))
    # the same cycles with HIP events around every kernel and around the all-reduce (out of `value`)
    ctx.timing_enable(True)
    kms = {}
    for i in range(min(steps, 50)):
        ctx.cycle_sharded(comm, pose(i), P)
        for name, ms in ctx.timings():
            if not name.startswith("host:"):
                kms.setdefault(name, []).append(ms)
    ctx.timing_enable(False)
    kernels_ms = {k: float(np.mean(v)) for k, v in kms.items()}
    shares = ranks.gather({"samples": count, "trig_rows": trig_rows, "single_launch": single, "kernels_ms": kernels_ms,
                           "winner": [bool(r.found), float(r.cost), int(r.raw_index), int(r.index), int(r.n_admissible)]})
    ctx.close()
    return {"scaling": "strong", "workload": f"{cfg}: {n_total} samples x {P} steps in all, dealt by trig row, scene 'mid'",
            "value": n_total * P * steps / el, "unit": "trajectory-steps/s", "ms_per_step": 1e3 * el / steps,
            "latency_p50_ms": p50, "steps": steps, "n_gpus": world, "n_admissible_global": int(r.n_admissible),
            "samples_per_rank": [s_["samples"] for s_ in shares], "trig_rows_per_rank": [s_["trig_rows"] for s_ in shares],
            # the ONE collective of a cycle: int64 x (2 + world x words per rank), ncclMin; its time by HIP events on the
            # launch stream of every rank (launch gaps included), the slowest rank's
            "exchange_record_bytes": 8 * (2 + world * ((max(s_["samples"] for s_ in shares) + 63) // 64)),
            "all_reduce_ms_max": max(s_["kernels_ms"].get("all_reduce", 0.0) for s_ in shares),
            "kernels_ms_rank0": shares[0]["kernels_ms"],
            "single_launch_per_rank": [s_["single_launch"] for s_ in shares],
            "ranks_agree": all(s_["winner"] == shares[0]["winner"] for s_ in shares),
            "winner": {"found": bool(r.found), "cost": float(r.cost), "raw_index": int(r.raw_index), "index": int(r.index)}}


def roofline_of(kernel_ms, count, P, map_side, S, O, scene="survey", cfg="cfg2"):
    """HBM roofline of the dominant kernel: algorithmic bytes of ONE launch (SURVEY
    8d: 16 B per trajectory-step + 20 B per sample + per-cycle constants; a launch
    of any kernel of the cycle covers all N x P steps) / its mean duration by HIP
    events on the launch stream."""
    dom = max(kernel_ms, key=lambda k: np.mean(kernel_ms[k]))
    dom_ms = float(np.mean(kernel_ms[dom]))
    bytes_launch = algorithmic_bytes(count, P, map_side, S, O)
    achieved = bytes_launch / (dom_ms * 1e-3) / 1e9
    traffic, traffic_src = pmc_traffic(dom, scene, cfg)
    out = {
        "bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
        "algorithmic_bytes_per_launch": bytes_launch, "avg_launch_ms": dom_ms,
        "note": "latency / VALU-issue bound path: the whole cycle moves ~7 MB (SURVEY 8d); the single-launch "
                "cycle keeps the poses in LDS and writes no float rows, so its HBM traffic is far below the "
                "algorithmic bytes it is priced with; valu_issue_frac (share of the chip's SIMD cycles that issue "
                "VALU work during the launch), salu_per_valu, lds_conflict_frac and critical_path_us (phase clocks "
                "of the slowest workgroup chain) say what binds it instead",
    }
    out.update(pmc_explain(dom, scene, cfg, dom_ms))
    return out


def scene_leg(ctx, cfg, scene, inp, vx, vy, om, P, S, pose, args):
    """One more bench line on the same context and lattice: another costmap."""
    import synthetic as syn

    base = syn.CONFIGS[cfg]
    pts = syn.scene_points(cfg, scene, seed=0)
    ctx.set_points(inp["state"], pts, inp["max_range"])
    n = len(vx)
    for i in range(args.warmup):
        r = ctx.cycle(pose(i), P)
    lat = []
    t0 = time.perf_counter()
    for i in range(args.steps):
        ts = time.perf_counter()
        r = ctx.cycle(pose(i), P)
        lat.append(time.perf_counter() - ts)
    elapsed = time.perf_counter() - t0
    ctx.timing_enable(True)
    kernel_ms = {}
    for i in range(min(args.steps, 500)):
        ctx.cycle(pose(i), P)
        for name, ms in ctx.timings():
            if not name.startswith("host:"):
                kernel_ms.setdefault(name, []).append(ms)
    ctx.timing_enable(False)
    r = ctx.cycle(pose(args.steps - 1), P)
    leg = {
        "metric": "trajectory-steps/s", "value": n * P * args.steps / elapsed, "unit": "trajectory-steps/s",
        "ms_per_step": 1e3 * elapsed / args.steps, "steps": args.steps,
        "latency_p50_ms": float(np.percentile(np.array(lat) * 1e3, 50)),
        "config": {"workload": f"{cfg} lattice ({n} x {P}) on scene '{scene}': {len(pts)} occupied cells, "
                               f"{int(r.n_admissible)} of {n} samples admissible", "scene": scene,
                   "n_admissible": int(r.n_admissible), "obstacles": int(len(pts))},
        "kernels_ms": {k: float(np.mean(v)) for k, v in kernel_ms.items()},
        "roofline": roofline_of(kernel_ms, n, P, base["map_side"], S, len(pts), scene, cfg),
    }
    if not args.no_cpu:
        leg["cpu_baseline"] = cpu_baseline(dict(inp, points=pts), vx, vy, om, pose(args.steps - 1), bool(r.found),
                                           float(r.cost), int(r.raw_index), args, max(2.0, args.cpu_seconds / 3))
    return leg


# class-level sample counts of SURVEY.md section 8 (max_linear_samples, max_angular_samples) per config
CLASS_SAMPLES = {"cfg1": (11, 11), "cfg2": (91, 91), "cfg3": (181, 181), "cfg5": (300, 215)}


def fresh_inputs_leg(kh, syn, ctx, cfg, inp, pose, args):
    """One REFERENCE controller cycle per step (DWA::findBestPath, include/controllers/dwa.h:183-230):
    new sensor data (octree rebuild + setPointScan -> kc_dwa_set_points), a new dynamic window and
    lattice (UpdateReachableVelocityRange + the lattice loops -> kc_dwa_sample_window), a new tracked
    segment (findTrackedPathSegment -> kc_dwa_set_tracked_segment), then roll-out + collision gate +
    costs + argmin (kc_dwa_cycle).  Nothing is resident between steps except buffers."""
    base = syn.CONFIGS[cfg]
    lim = kh.make_limits(syn.LIMITS["vx"], syn.LIMITS["vy"], syn.LIMITS["omega"])
    max_lin, max_ang = CLASS_SAMPLES[cfg]
    P, S, O = inp["P"], len(inp["seg_xyz"]), len(inp["points"])
    cur = lambda i: (0.5 + 0.002 * ((i % 5) - 2), 0.0, 0.01 * ((i % 3) - 1))   # the window moves every cycle

    # (the arrays as a C++ caller holds them: contiguous float32, no per-call conversion in the Python binding)
    seg = np.asarray(inp["seg_xyz"], np.float32)
    sx, sy, sz = (np.ascontiguousarray(seg[:, k]) for k in range(3))
    sacc = np.ascontiguousarray(inp["acc_at_seg"], np.float32)
    pts = np.ascontiguousarray(inp["points"], np.float32)

    def step4(i):  # the four entries one by one (what rounds 1-3 timed)
        st = pose(i)
        ctx.sample_window(base["ctr"], lim, cur(i), max_lin, max_ang, want_list=False)
        ctx.set_points(st, pts, inp["max_range"])
        ctx.set_tracked_segment_columns(sx, sy, sz, sacc, inp["ref_len"])
        return ctx.cycle(st, P)

    def step(i):   # the same cycle through ONE entry (kc_dwa_find_best_path = DWA::findBestPath, dwa.h:183-230)
        return ctx.find_best_path(pose(i), P, window=(base["ctr"], lim, cur(i), max_lin, max_ang), points=pts,
                                  max_sensor_range=inp["max_range"], segment=(seg, sacc, inp["ref_len"]))

    n = int(ctx.sample_window(base["ctr"], lim, cur(0), max_lin, max_ang, want_list=False))
    # as the top-level line (--fresh) the leg runs exactly --steps; beside the headline it is capped
    steps, warm = (args.steps, args.warmup) if args.fresh else (min(args.steps, 1000), min(args.warmup, 100))
    for i in range(warm):
        step4(i)
    t4 = time.perf_counter()
    for i in range(steps):
        r4 = step4(i)
    four_calls_ms = 1e3 * (time.perf_counter() - t4) / steps
    for i in range(warm):
        step(i)
    lat = []
    t0 = time.perf_counter()
    for i in range(steps):
        ts = time.perf_counter()
        r = step(i)
        lat.append(time.perf_counter() - ts)
    elapsed = time.perf_counter() - t0
    if args.fresh and args.dump_outputs:
        write_outputs(args.dump_outputs, cycle_outputs(ctx, r))
    ctx.timing_enable(True)
    kernel_ms = {}
    for i in range(min(steps, 300)):
        st = pose(i)
        ctx.sample_window(base["ctr"], lim, cur(i), max_lin, max_ang, want_list=False)
        ctx.set_points(st, pts, inp["max_range"])
        for name, ms in ctx.timings():
            if not name.startswith("host:"):
                kernel_ms.setdefault(name, []).append(ms)
        ctx.set_tracked_segment_columns(sx, sy, sz, sacc, inp["ref_len"])
        ctx.cycle(st, P)
        for name, ms in ctx.timings():
            if not name.startswith("host:"):
                kernel_ms.setdefault(name, []).append(ms)
    ctx.timing_enable(False)
    last_i = steps - 1
    r = step(last_i)
    leg = {
        "metric": "trajectory-steps/s", "value": n * P * steps / elapsed, "unit": "trajectory-steps/s",
        "ms_per_step": 1e3 * elapsed / steps, "steps": steps, "warmup": warm,
        "latency_p50_ms": float(np.percentile(np.array(lat) * 1e3, 50)),
        "entry": "kc_dwa_find_best_path (one C-ABI call per cycle: window + points + segment + cycle)",
        "four_calls_ms_per_step": four_calls_ms,
        "four_calls_same_winner": bool((r4.found, r4.raw_index, r4.index, r4.n_admissible) ==
                                       (r.found, r.raw_index, r.index, r.n_admissible) and np.float32(r4.cost) == np.float32(r.cost)),
        "config": {"workload": f"{cfg}, one reference controller cycle per step: kc_dwa_sample_window (max_linear_samples "
                               f"{max_lin}, max_angular_samples {max_ang}: {n} samples) + kc_dwa_set_points ({O} points: "
                               f"voxel set + obstacle list) + kc_dwa_set_tracked_segment ({S} points) + kc_dwa_cycle "
                               f"({n} x {P} steps), scene '{inp['scene']}', {int(r.n_admissible)} of {n} admissible at the last pose",
                   "samples": n, "points": P, "n_admissible": int(r.n_admissible), "reference": "controllers/dwa.h:183-230"},
        "kernels_ms": {k: float(np.mean(v)) for k, v in kernel_ms.items()},
        "launches_per_step": len(kernel_ms),
        # (the counter passes of THIS leg: profiles/*_<cfg>_fresh_pmc_{hbm,sq}.json, collected with --fresh)
        "roofline": roofline_of({k: v for k, v in kernel_ms.items()}, n, P, base["map_side"], S, O, "fresh", cfg),
        "winner": {"found": bool(r.found), "cost": float(r.cost), "raw_index": int(r.raw_index), "index": int(r.index)},
    }
    if not args.no_cpu:
        leg["cpu_baseline"] = cpu_baseline_fresh(syn, inp, base["ctr"], cur(last_i), max_lin, max_ang, pose(last_i), r, args,
                                                 max(3.0, args.cpu_seconds / 2))
    leg["moving_window"] = moving_window_block(ctx, base, lim, max_lin, max_ang, pose, P, pts, seg, sacc, inp, min(steps, 1500))
    ctx.sample_window(base["ctr"], lim, cur(last_i), max_lin, max_ang, want_list=False)
    return leg


def moving_window_block(ctx, base, lim, max_lin, max_ang, pose, P, pts, seg, sacc, inp, steps):
    """The same reference cycle with a velocity that WANDERS (a bounded random walk: what a closed loop's own commands do
    to it).  The loop above moves its window among values that keep the lattice's index pattern; a robot changes pattern
    in every second cycle (an axis gains or loses a value, a value crosses |v| = kMinVel), and a new pattern costs the
    host a rebuild of the roll-out's walking orders.  Not `value`: a second reading of the
    same path."""
    rng = np.random.default_rng(1)
    vx, om, lat, counts = 0.3, 0.0, [], []
    h0, b0 = ctx.get_option("pattern_hits"), ctx.get_option("pattern_builds")
    for i in range(steps + 100):
        vx = float(np.clip(vx + rng.normal(0, 0.02), -0.2, 1.0))
        om = float(np.clip(om + rng.normal(0, 0.05), -1.0, 1.0))
        ts = time.perf_counter()
        r = ctx.find_best_path(pose(i), P, window=(base["ctr"], lim, (vx, 0.0, om), max_lin, max_ang), points=pts,
                               max_sensor_range=inp["max_range"], segment=(seg, sacc, inp["ref_len"]))
        if i >= 100:
            lat.append(time.perf_counter() - ts)
            counts.append(int(r.n_samples))
    lat = np.array(lat) * 1e3
    return {"what": "kc_dwa_find_best_path under a bounded random walk of the current velocity (sigma 0.02 m/s, 0.05 rad/s per cycle)",
            "steps": steps, "ms_per_step": float(lat.mean()), "latency_p50_ms": float(np.percentile(lat, 50)),
            "latency_p90_ms": float(np.percentile(lat, 90)), "latency_p99_ms": float(np.percentile(lat, 99)),
            "sample_count_changes": int(np.sum(np.diff(counts) != 0)),
            "patterns_found_on_device": int(ctx.get_option("pattern_hits") - h0),
            "patterns_built": int(ctx.get_option("pattern_builds") - b0)}


def cpu_baseline_fresh(syn, inp, ctr, cur_vel, max_lin, max_ang, state, r, args, seconds):
    """The oracle's whole reference cycle on this host's cores: window + lattice, voxel-set build
    (CollisionChecker::updateSensorData restated), setPointScan, roll-out + collision + costs + argmin."""
    from oracle import ko

    rb = inp["robot"]
    lim = ko.make_limits(syn.LIMITS["vx"], syn.LIMITS["vy"], syn.LIMITS["omega"])
    P = inp["P"]
    ncores = usable_cpus()

    def inputs():
        vx, vy, om = ko.sample_velocities(ctr, lim, cur_vel, inp["dt"], max_lin, max_ang)
        coll = ko.Collision(rb["shape"], rb["dims"], (0, 0, 0), (0, 0, 0, 1), inp["octree_res"])
        coll.update_state(*state[:3])
        coll.update_points(inp["points"], True)
        ox, oy = ko.obstacles_from_points((0, 0, 0), (0, 0, 0, 1), state, inp["points"])
        ci = ko.CostInputs(inp["seg_xyz"], 0, inp["acc_at_seg"], inp["ref_len"], np.stack([ox, oy], 1),
                           np.float32(inp["max_range"]) / np.float32(3.0), inp["acc_limits"],
                           ko.make_weights(*inp["weights"]))
        return vx, vy, om, coll, ci

    t0 = time.perf_counter()
    vx, vy, om, coll, ci = inputs()
    t_in = time.perf_counter() - t0
    n = len(vx)
    t0 = time.perf_counter()
    oi, oc, na = ko.baseline_cycle(coll, ci, state, inp["dt"], P, vx, vy, om, threads=ncores)
    t_mt = time.perf_counter() - t0
    parity = bool((oi >= 0) == bool(r.found) and (not r.found or (oi == int(r.raw_index) and
                                                                  np.float32(oc) == np.float32(r.cost))))
    stride = max(1, int(np.ceil(t_mt * ncores / max(seconds, 0.5))))
    t0 = time.perf_counter()
    cycles = 0
    t_inputs = []
    while cycles < (3 if stride == 1 else 1) or (time.perf_counter() - t0 < seconds and cycles < 1000):
        ti = time.perf_counter()
        vx, vy, om, coll, ci = inputs()
        t_inputs.append(time.perf_counter() - ti)
        ko.baseline_cycle(coll, ci, state, inp["dt"], P, vx[::stride], vy[::stride], om[::stride], threads=1)
        cycles += 1
    t_all = (time.perf_counter() - t0) / cycles
    t_inp = float(np.mean(t_inputs))
    # a full cycle = the per-cycle inputs once + every sample: the strided samples scaled back up
    t_cycle = t_inp + (t_all - t_inp) * stride
    return {
        "value": n * P / t_cycle, "unit": "trajectory-steps/s", "cores": 1, "kind": "port",
        "sample": f"{cycles} cycles on 1 thread: window + lattice + voxel set + obstacle list every cycle ({t_inp * 1e3:.2f} ms), "
                  f"every {stride}th of the {n} samples rolled out and scored ({(t_all - t_inp) * 1e3:.1f} ms), scaled to all "
                  f"samples: {t_cycle * 1e3:.1f} ms per reference cycle",
        "inputs_ms": t_inp * 1e3, "first_inputs_ms": t_in * 1e3,
        "all_cores": {"value": n * P / (t_in + t_mt), "cores": ncores, "seconds": t_in + t_mt,
                      "sample": "inputs on one core + 1 full cycle on all"},
        "gpu_matches_cpu_winner": parity,
        "cpu_winner": {"raw_index": int(oi), "cost": float(oc), "n_admissible": int(na)},
    }


def laserscan_leg(ctx, cfg, inp, vx, vy, om, P, S, pose, args, beams=1440):
    """The same lattice with LaserScan input (the reference test's own input form, tests/test_controllers.py:213):
    a room-like scan of `beams` beams -- walls metres from every trajectory point, the octree in the sensor frame
    (collision_check.h:99-117), the obstacle list from CostEvaluator::setPointScan(LaserScan)."""
    import synthetic as syn

    base = syn.CONFIGS[cfg]
    ang = np.linspace(-np.pi, np.pi, beams, endpoint=False)
    rng = 4.0 + 1.5 * np.cos(5 * ang)
    ctx.set_scan(inp["state"], rng, ang, inp["max_range"])
    n = len(vx)
    for i in range(args.warmup):
        r = ctx.cycle(pose(i), P)
    lat = []
    t0 = time.perf_counter()
    for i in range(args.steps):
        ts = time.perf_counter()
        r = ctx.cycle(pose(i), P)
        lat.append(time.perf_counter() - ts)
    elapsed = time.perf_counter() - t0
    if args.scan and args.dump_outputs:
        write_outputs(args.dump_outputs, cycle_outputs(ctx, r))
    ctx.timing_enable(True)
    kernel_ms = {}
    for i in range(min(args.steps, 500)):
        ctx.cycle(pose(i), P)
        for name, ms in ctx.timings():
            if not name.startswith("host:"):
                kernel_ms.setdefault(name, []).append(ms)
    ctx.timing_enable(False)
    fresh = []
    for i in range(200):  # new scan every cycle (the table of the scan is rebuilt every time)
        ts = time.perf_counter()
        ctx.set_scan(inp["state"], rng + 0.01 * (i % 9), ang, inp["max_range"])
        ctx.cycle(pose(i), P)
        fresh.append(time.perf_counter() - ts)
    ctx.set_scan(inp["state"], rng, ang, inp["max_range"])
    r = ctx.cycle(pose(args.steps - 1), P)
    leg = {
        "metric": "trajectory-steps/s", "value": n * P * args.steps / elapsed, "unit": "trajectory-steps/s",
        "ms_per_step": 1e3 * elapsed / args.steps, "steps": args.steps,
        "latency_p50_ms": float(np.percentile(np.array(lat) * 1e3, 50)),
        "set_scan_and_cycle_ms": float(np.median(fresh) * 1e3),
        "config": {"workload": f"{cfg} lattice ({n} x {P}) with LaserScan input: {beams} beams, room-like ranges 2.5-5.5 m, "
                               f"{int(r.n_admissible)} of {n} samples admissible", "beams": beams,
                   "n_admissible": int(r.n_admissible)},
        "kernels_ms": {k: float(np.mean(v)) for k, v in kernel_ms.items()},
        "roofline": roofline_of(kernel_ms, n, P, base["map_side"], S, beams, "scan", cfg),
    }
    if not args.no_cpu:
        from oracle import ko

        rb = inp["robot"]
        state = pose(args.steps - 1)
        coll = ko.Collision(rb["shape"], rb["dims"], (0, 0, 0), (0, 0, 0, 1), inp["octree_res"])
        coll.update_state(*inp["state"][:3])
        coll.update_scan(rng, ang)
        ox, oy = ko.obstacles_from_scan((0, 0, 0), (0, 0, 0, 1), inp["state"], rng, ang)
        ci = ko.CostInputs(inp["seg_xyz"], 0, inp["acc_at_seg"], inp["ref_len"], np.stack([ox, oy], 1),
                           np.float32(inp["max_range"]) / np.float32(3.0), inp["acc_limits"], ko.make_weights(*inp["weights"]))
        ncores = usable_cpus()
        t0 = time.perf_counter()
        oi, oc, na = ko.baseline_cycle(coll, ci, state, inp["dt"], P, vx, vy, om, threads=ncores)
        t_mt = time.perf_counter() - t0
        stride = max(1, int(np.ceil(t_mt * ncores / 4.0)))
        t0 = time.perf_counter()
        ko.baseline_cycle(coll, ci, state, inp["dt"], P, vx[::stride], vy[::stride], om[::stride], threads=1)
        t_1 = time.perf_counter() - t0
        leg["cpu_baseline"] = {
            "value": len(vx[::stride]) * P / t_1, "unit": "trajectory-steps/s", "cores": 1, "kind": "port",
            "sample": f"1 cycle over every {stride}th of the {n} samples on 1 thread: {t_1 * 1e3:.0f} ms",
            "all_cores": {"value": n * P / t_mt, "cores": ncores, "seconds": t_mt, "sample": "1 full cycle"},
            "gpu_matches_cpu_winner": bool((oi >= 0) == bool(r.found) and (not r.found or (
                oi == int(r.raw_index) and np.float32(oc) == np.float32(r.cost)))),
            "cpu_winner": {"raw_index": int(oi), "cost": float(oc), "n_admissible": int(na)}}
    return leg


def extras(ctx, inp, P, pose):
    """Not part of `value`: what the per-cycle input updates cost (sensor data,
    tracked segment, mapper hand-off)."""
    def med(fn, n):
        ts = []
        for i in range(n):
            t0 = time.perf_counter()
            fn(i)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts) * 1e3)

    pts = np.asarray(inp["points"], dtype=np.float32).reshape(-1, 3)
    out = {
        "set_points_ms": med(lambda i: ctx.set_points(inp["state"], inp["points"], inp["max_range"]), 20),
        "set_tracked_segment_ms": med(lambda i: ctx.set_tracked_segment(inp["seg_xyz"], inp["acc_at_seg"],
                                                                         inp["ref_len"]), 20),
    }
    def fresh_inputs_cycle(i):
        ctx.set_points(inp["state"], inp["points"], inp["max_range"])
        ctx.set_tracked_segment(inp["seg_xyz"], inp["acc_at_seg"], inp["ref_len"])
        ctx.cycle(pose(i), P)

    # a controller step with new sensor data and a new tracked segment every time
    out["update_and_cycle_ms"] = med(fresh_inputs_cycle, 100)
    # the same with the reference path resident on the device: only the window moves
    ctx.set_path(inp["seg_xyz"], inp["acc_at_seg"], inp["ref_len"])

    def fresh_inputs_window_cycle(i):
        ctx.set_points(inp["state"], inp["points"], inp["max_range"])
        ctx.set_tracked_window(0, len(inp["seg_xyz"]))
        return ctx.cycle(pose(i), P)

    ra = ctx.cycle(pose(0), P)
    rb = fresh_inputs_window_cycle(0)
    out["update_and_cycle_resident_path_ms"] = med(fresh_inputs_window_cycle, 100)
    out["resident_path_same_result"] = bool(ra.raw_index == rb.raw_index and np.float32(ra.cost) == np.float32(rb.cost))
    ctx.set_tracked_segment(inp["seg_xyz"], inp["acc_at_seg"], inp["ref_len"])
    out["mapper_handoff"] = handoff_extra(ctx, inp, P, pose, med)
    ctx.set_points(inp["state"], inp["points"], inp["max_range"])
    r = ctx.cycle(pose(0), P)
    out["n_admissible"] = int(r.n_admissible)
    return out


def handoff_extra(ctx, inp, P, pose, med):
    """scan -> grid -> controller, once with the grid staying
    on the device (OCCUPIED cells extracted there) and once the reference's way
    (grid to the host, point list extracted there, list back to the device)."""
    import kompass_hip as kh
    import synthetic as syn

    side, res, beams = 500, 0.05, 4096
    ang, rng = syn.dense_scan(beams, 0.9)
    m = kh.MapperContext(side, side, res, (0, 0, 0), 0.0, beams)
    c0 = side // 2 - 1
    seg = lambda: ctx.set_tracked_segment(inp["seg_xyz"], inp["acc_at_seg"], inp["ref_len"])

    def on_device(i):
        m.scan_to_grid_device(ang, rng)
        ctx.set_grid_from_mapper(inp["state"], m, inp["max_range"])
        seg()
        return ctx.cycle(pose(i), P)

    def through_host(i):
        g = m.scan_to_grid(ang, rng)
        ii, jj = np.nonzero(g == 100)
        pts = np.zeros((len(ii), 3), np.float32)
        pts[:, 0] = (ii - c0).astype(np.float32) * np.float32(res)
        pts[:, 1] = (jj - c0).astype(np.float32) * np.float32(res)
        ctx.set_points(inp["state"], pts, inp["max_range"])
        seg()
        return ctx.cycle(pose(i), P)

    ra, rb = on_device(0), through_host(0)
    same = bool(ra.found == rb.found and ra.raw_index == rb.raw_index and
                np.float32(ra.cost) == np.float32(rb.cost) and ra.n_admissible == rb.n_admissible)
    return {"on_device_ms": med(on_device, 100), "through_host_ms": med(through_host, 30),
            "same_result": same, "n_admissible": int(ra.n_admissible),
            "what": f"{beams}-beam scan -> {side}x{side} grid -> sensor update -> segment -> cycle"}


def usable_cpus():
    """CPUs this process may really use: the affinity mask, capped by the cgroup quota
    (the GPU boxes show 256 hardware threads and allow 16)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    return max(1, n)


def cpu_baseline(inp, vx, vy, om, state, found, cost, raw, args, seconds):
    """The oracle (a port of the reference CPU path, `kind: port`) timed on this
    host's cores on a bounded sample of the same workload, 1 thread (the
    reference default max_num_threads=1, dwa.py:131) and all cores; also checks
    the GPU winner of the last timed cycle against it."""
    from oracle import ko

    rb = inp["robot"]
    coll = ko.Collision(rb["shape"], rb["dims"], (0, 0, 0), (0, 0, 0, 1), inp["octree_res"])
    coll.update_state(*inp["state"][:3])
    coll.update_points(inp["points"], True)
    ox, oy = ko.obstacles_from_points((0, 0, 0), (0, 0, 0, 1), inp["state"], inp["points"])
    ci = ko.CostInputs(inp["seg_xyz"], 0, inp["acc_at_seg"], inp["ref_len"], np.stack([ox, oy], 1),
                       np.float32(inp["max_range"]) / np.float32(3.0), inp["acc_limits"],
                       ko.make_weights(*inp["weights"]))
    P = inp["P"]
    ncores = usable_cpus()
    n = len(vx)
    # full-batch parity of the last GPU cycle, all cores
    t0 = time.perf_counter()
    oi, oc, na = ko.baseline_cycle(coll, ci, state, inp["dt"], P, vx, vy, om, threads=ncores)
    t_mt = time.perf_counter() - t0
    parity = bool((oi >= 0) == found and (not found or (oi == raw and np.float32(oc) == np.float32(cost))))
    # 1-thread timing on a bounded sample: whole cycles until ~`seconds` (a cycle over every
    # `stride`-th sample when a full one would take longer than that: the all-core cycle above
    # tells how long)
    stride = max(1, int(np.ceil(t_mt * ncores / max(seconds, 0.5))))
    svx, svy, som = vx[::stride], vy[::stride], om[::stride]
    t0 = time.perf_counter()
    cycles = 0
    while cycles < (3 if stride == 1 else 1) or (time.perf_counter() - t0 < seconds and cycles < 1000):
        ko.baseline_cycle(coll, ci, state, inp["dt"], P, svx, svy, som, threads=1)
        cycles += 1
    t_1 = (time.perf_counter() - t0) / cycles
    return {
        "value": len(svx) * P / t_1, "unit": "trajectory-steps/s", "cores": 1, "kind": "port",
        "sample": f"{cycles} cycles over {len(svx)} of the {n} samples (every {stride}th) x {P} steps, "
                  f"{t_1 * 1e3:.1f} ms per cycle on 1 thread",
        "all_cores": {"value": n * P / t_mt, "cores": ncores, "seconds": t_mt,
                      "sample": f"1 full cycle ({n} samples)"},
        "gpu_matches_cpu_winner": parity, "cpu_winner": {"raw_index": int(oi), "cost": float(oc),
                                                         "n_admissible": int(na)},
        "note": "oracle uses a hashed voxel set instead of FCL's octree traversal, so it is faster than the "
                "real reference CPU path; the ratio is conservative",
    }


def mapper_bench(args):
    """BASELINE configs[3]: 4096-beam scan into a 1000x1000 grid (not the
    default bench line; `--mapper`)."""
    import kompass_hip as kh
    import synthetic as syn
    from oracle import ko

    H = W = 1000
    n = 4096
    ang, rng = syn.dense_scan(n, 4.0)
    m = kh.MapperContext(H, W, 0.05, (0, 0, 0), 0.0, n)
    scans = [rng * (1.0 + 0.01 * ((i % 5) - 2)) for i in range(8)]
    for i in range(args.warmup):
        m.scan_to_grid_device(ang, scans[i % 8])
        m.sync()
    lat, t_call = [], []
    t0 = time.perf_counter()
    for i in range(args.steps):
        ta = time.perf_counter()
        m.scan_to_grid_device(ang, scans[i % 8])
        tb = time.perf_counter()
        m.sync()
        tc = time.perf_counter()
        lat.append(tc - ta)
        t_call.append(tb - ta)
    el = time.perf_counter() - t0
    lat_us, call_us = np.array(lat) * 1e6, np.array(t_call) * 1e6
    # same scans again with HIP events around every kernel (roofline leg; the
    # events stay out of `value`)
    m.timing_enable(True)
    kms = {}
    for i in range(args.steps):
        m.scan_to_grid_device(ang, scans[i % 8])
        m.sync()
        for k, v in m.timings():
            kms.setdefault(k, []).append(v)
    m.timing_enable(False)
    t1 = time.perf_counter()
    for i in range(args.steps):
        g = m.scan_to_grid(ang, scans[i % 8])
    el_host = time.perf_counter() - t1
    t2 = time.perf_counter()
    want = ko.scan_to_grid(H, W, 0.05, (0, 0, 0), 0.0, ang, scans[(args.steps - 1) % 8])
    t_cpu = time.perf_counter() - t2
    ray_cells = int((want >= 0).sum())
    bytes_scan = 4 * H * W + 12 * n + 12 * ray_cells
    dom = max(kms, key=lambda k: np.mean(kms[k]))
    dom_ms = float(np.mean(kms[dom]))
    kernels_sum_us = float(sum(np.mean(v) for v in kms.values()) * 1e3)
    return {
        "metric": "scans/s", "value": args.steps / el, "unit": "scans/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1e3 * el / args.steps, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "int32 grid / f32 endpoints", "data": "synthetic",
        "config": {"workload": "cfg4: LocalMapper 4096 beams -> 1000x1000@0.05 grid, grid resident on device"},
        "latency_p50_ms": float(np.percentile(lat_us, 50)) * 1e-3, "latency_min_ms": float(lat_us.min()) * 1e-3,
        "latency_max_ms": float(lat_us.max()) * 1e-3,
        # where a scan's wall time goes: the call (ranges over the BAR + the launches) returns, then kc_mapper_sync
        # polls the word the last endpoints workgroup posts into pinned memory: kernels_sum is the kernels' own run
        # time by HIP events, the rest of call + wait is launch / dispatch latency in front of and between them
        # (BENCH_r03: 42 us per scan on the driver's box against 27 on the builder's with 24 us of kernels on both)
        "host_phases_us": {"call_p50": float(np.percentile(call_us, 50)),
                           "sync_wait_p50": float(np.percentile(lat_us - call_us, 50)),
                           "kernels_sum": kernels_sum_us},
        "pcie_inclusive_scans_per_s": args.steps / el_host,
        "kernels_ms": {k: float(np.mean(v)) for k, v in kms.items()},
        "roofline": dict({"bound": "hbm", "kernel": dom, "achieved": bytes_scan / (dom_ms * 1e-3) / 1e9,
                          "peak": HBM_PEAK_GBS, "unit": "GB/s",
                          "frac": bytes_scan / (dom_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                          "traffic": pmc_traffic(dom, "mapper", "cfg4")[0], "traffic_source": pmc_traffic(dom, "mapper", "cfg4")[1],
                          "algorithmic_bytes_per_launch": bytes_scan, "avg_launch_ms": dom_ms,
                          "note": "bytes of one scan (SURVEY 8d: clear 4 HW + beams 12 B + 12 B per traversed cell) over the "
                                  "slowest of its kernels; store-issue bound (three ordered passes of scattered 4-byte stores)"},
                         **pmc_explain(dom, "mapper", "cfg4", dom_ms)),
        "cpu_baseline": {"value": 1.0 / t_cpu, "unit": "scans/s", "cores": 1, "kind": "port",
                         "sample": "1 scan", "grid_matches": bool(np.array_equal(g, want))},
    }


def bayes_mapper_bench(args):
    """SURVEY 8f rank 3 (not the default bench line; `--mapper --bayes`): one
    step of the Bayesian mapping loop at cfg4 size -- warp the previous
    probability grid to the new pose, scan with the Bayesian update, feed the
    probabilities back -- everything resident on the device.  The reference's
    own CPU mapper benchmark times scanToGridBaysian
    (benchmark_runner.cpp:207-213)."""
    import kompass_hip as kh
    import synthetic as syn
    from oracle import ko

    H = W = 1000
    n = 4096
    params = dict(p_prior=0.6, p_occupied=0.9, p_empty=0.1, range_sure=0.1, range_max=20.0, wall_size=0.2)
    ang, rng = syn.dense_scan(n, 4.0)
    m = kh.MapperContext(H, W, 0.05, (0, 0, 0), 0.0, n)
    m.enable_bayes(**params)
    scans = [rng * (1.0 + 0.01 * ((i % 5) - 2)) for i in range(8)]
    pose = lambda i: ((0.01 * (i % 7), -0.005 * (i % 5)), 0.002 * (i % 11))

    def step(i):
        m.get_previous_grid_in_current_pose(*pose(i))
        m.scan_to_grid_baysian_device(ang, scans[i % 8])
        m.set_previous_prob(None)
        m.sync()

    for i in range(args.warmup):
        step(i)
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    m.set_stream(None)  # drains the stream: the last feedback copy is inside the timed region
    el = time.perf_counter() - t0
    m.timing_enable(True)
    kms = {}
    for i in range(args.steps):
        m.get_previous_grid_in_current_pose(*pose(i))
        for k, v in m.timings():
            kms.setdefault(k, []).append(v)
        m.scan_to_grid_baysian_device(ang, scans[i % 8])
        m.sync()
        for k, v in m.timings():
            kms.setdefault(k, []).append(v)
    m.timing_enable(False)
    # parity + CPU baseline on the same three steps from a fresh state
    m2 = kh.MapperContext(H, W, 0.05, (0, 0, 0), 0.0, n)
    m2.enable_bayes(**params)
    o = ko.BayesMapper(H, W, 0.05, (0, 0, 0), 0.0, **params)
    t2 = time.perf_counter()
    for i in range(3):
        o.get_previous_grid_in_current_pose(*pose(i))
        want_g, want_p = o.scan_to_grid_baysian(ang, scans[i % 8])
        o.set_previous(want_p)
    t_cpu = (time.perf_counter() - t2) / 3
    for i in range(3):
        m2.get_previous_grid_in_current_pose(*pose(i))
        got_g, got_p = m2.scan_to_grid_baysian(ang, scans[i % 8])
        m2.set_previous_prob(None)
    same = bool(np.array_equal(got_g, want_g) and
                np.array_equal(np.ascontiguousarray(got_p).view(np.uint32),
                               np.ascontiguousarray(want_p).view(np.uint32)))
    ray_cells = int((want_g >= 0).sum())
    cells = H * W
    # per step: warp 2x4 B/cell, clear 4, tags read+reset, previous read, prob write (4 each where
    # touched), feedback copy 2x4, plus the ray read-modify-writes of the plain scan
    bytes_step = cells * (8 + 4 + 4 + 4 + 8) + 12 * n + ray_cells * (12 + 8 + 4)
    dom = max(kms, key=lambda k: np.mean(kms[k]))
    dom_ms = float(np.mean(kms[dom]))
    dom_bytes = {"warp_kernel": 8 * cells, "grid_clear": 4 * cells, "rays_kernel": 20 * ray_cells + 12 * n,
                 "bayes_cells_kernel": 8 * cells + 12 * ray_cells, "endpoints_kernel": 16 * n}.get(dom, bytes_step)
    return {
        "metric": "mapping steps/s", "value": args.steps / el, "unit": "steps/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1e3 * el / args.steps, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32 probabilities (f64 odds) / int32 grid",
        "data": "synthetic",
        "config": {"workload": "cfg4 grid, Bayesian loop: warp previous grid + 4096-beam Bayesian scan + "
                               "feedback, 1000x1000@0.05, grids resident on device"},
        "kernels_ms": {k: float(np.mean(v)) for k, v in kms.items()},
        "roofline": {"bound": "hbm", "kernel": dom, "achieved": dom_bytes / (dom_ms * 1e-3) / 1e9,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": dom_bytes / (dom_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                     "traffic": None},
        "cpu_baseline": {"value": 1.0 / t_cpu, "unit": "steps/s", "cores": 1, "kind": "port",
                         "sample": "3 steps", "grids_match": same},
    }


def pointcloud_bench(args):
    """SURVEY 8f rank 1 (not the default bench line; `--pointcloud`): 1M-point
    PointCloud2 buffer resident on the device -> 2048-bin laserscan."""
    import torch

    import kompass_hip as kh
    from oracle import ko

    n, bins, step = 1_000_000, 2048, 16
    rng = np.random.default_rng(0)
    xyz = np.zeros((n, 4), np.float32)
    xyz[:, 0] = rng.uniform(-30, 30, n)
    xyz[:, 1] = rng.uniform(-30, 30, n)
    xyz[:, 2] = rng.uniform(0.0, 1.0, n)
    host = xyz.reshape(-1).view(np.int8)
    dev = torch.from_numpy(host.copy()).cuda()
    torch.cuda.synchronize()
    ctx = kh.CloudContext(max_bytes=host.size, max_bins=bins)
    call = lambda: ctx.to_laserscan(None, step, n * step, 1, n, 0, 4, 8, 25.0, 0.0, 1.0, num_bins=bins,
                                    device_ptr=dev.data_ptr(), nbytes=host.size)
    for _ in range(args.warmup):
        got = call()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        got = call()
    el = time.perf_counter() - t0
    # same calls again with HIP events around the kernels (roofline leg)
    ctx.timing_enable(True)
    kms = []
    for _ in range(args.steps):
        got = call()
        kms += [ms for name, ms in ctx.timings() if name == "cloud_bins_kernel"]
    ctx.timing_enable(False)
    t1 = time.perf_counter()
    got_h = ctx.to_laserscan(host, step, n * step, 1, n, 0, 4, 8, 25.0, 0.0, 1.0, num_bins=bins)
    el_host = time.perf_counter() - t1
    t2 = time.perf_counter()
    want = ko.pointcloud_to_laserscan(host, step, n * step, 1, n, 0, 4, 8, 25.0, 0.0, 1.0, num_bins=bins)
    t_cpu = time.perf_counter() - t2
    k_ms = float(np.mean(kms))
    bytes_launch = 12 * n + 8 * bins  # x, y, z of every point read once + one double per bin
    return {
        "metric": "points/s", "value": n * args.steps / el, "unit": "points/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1e3 * el / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32 in / f64 ranges", "data": "synthetic",
        "config": {"workload": f"point cloud -> laserscan: {n} points (16-byte records, device resident), {bins} bins"},
        "kernels_ms": {"cloud_bins_kernel": k_ms},
        "roofline": {"bound": "hbm", "kernel": "cloud_bins_kernel", "achieved": bytes_launch / (k_ms * 1e-3) / 1e9,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": bytes_launch / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                     "traffic": None, "algorithmic_bytes_per_launch": bytes_launch, "avg_launch_ms": k_ms},
        "pcie_inclusive_ms": 1e3 * el_host,
        "rebinned_on_host": ctx.last_rebinned(),
        "cpu_baseline": {"value": n / t_cpu, "unit": "points/s", "cores": 1, "kind": "port",
                         "sample": f"one {n}-point cloud, {t_cpu * 1e3:.1f} ms"},
        "matches_cpu": bool(np.array_equal(got.view(np.uint64), want.view(np.uint64))
                            and np.array_equal(got_h.view(np.uint64), want.view(np.uint64))),
    }


def ref_cost5k_inputs():
    """CostEvaluator_5k_Trajs of the reference's benchmark suite (benchmark_runner.cpp:152-185)."""
    import synthetic as syn
    from oracle import ko  # Path preparation only (host glue: interpolate + segment)

    r = syn.REF_COST5K
    p = ko.Path(r["path_points"])
    p.interpolate(r["interpolation"])
    p.segment(r["segment_length"], r["max_segment_points"])
    s0, s1 = p.segment_range(0)
    seg = np.stack([p.x[s0:s1 + 1], p.y[s0:s1 + 1], p.z[s0:s1 + 1]], axis=1).astype(np.float32)
    px, py, vel = syn.ref_cost5k_samples()
    return dict(px=px, py=py, vel=vel, seg=seg, s0=s0, acc=np.asarray(p.acc, np.float32).copy(),
                total=float(p.total_length), acc_limits=r["acc_limits"], weights=r["weights"])


def ref_cost5k_bench(args):
    """`--ref cost5k`: the reference's published CostEvaluator workload -- 5001 trajectories x 1000
    points with velocity profiles against a 1000-point segment, weights path = goal = smoothness =
    jerk = 1 -- through kc_cost_upload (once) + kc_cost_evaluate_resident (timed)."""
    import kompass_hip as kh
    import synthetic as syn
    from oracle import ko

    w = ref_cost5k_inputs()
    N, P = w["px"].shape
    S = len(w["seg"])
    ctx = kh.DwaContext(syn.CYLINDER, [0.1, 0.4], max_samples=N, max_points=P, max_segment=S,
                        acc_limits=w["acc_limits"])
    ctx.set_weights(kh.make_weights(*w["weights"]))
    ctx.set_tracked_segment(w["seg"], w["acc"][w["s0"]:w["s0"] + S], w["total"])
    ctx.cost_upload(w["px"], w["py"], w["vel"])
    steps, warm = args.steps, args.warmup
    for _ in range(warm):
        ctx.cost_evaluate_resident(with_costs=False)
    lat = []
    t0 = time.perf_counter()
    for _ in range(steps):
        ts = time.perf_counter()
        r = ctx.cost_evaluate_resident(with_costs=False)
        lat.append(time.perf_counter() - ts)
    el = time.perf_counter() - t0
    ctx.timing_enable(True)
    kms = {}
    for _ in range(min(steps, 50)):
        ctx.cost_evaluate_resident(with_costs=False)
        for name, ms in ctx.timings():
            if not name.startswith("host:"):
                kms.setdefault(name, []).append(ms)
    ctx.timing_enable(False)
    r, costs = ctx.cost_evaluate_resident()
    # PCIe-inclusive: samples uploaded on every call, like the reference's device path does
    t1 = time.perf_counter()
    for _ in range(5):
        ctx.cost_evaluate(w["px"], w["py"], w["vel"])
    el_pcie = (time.perf_counter() - t1) / 5
    ms = 1e3 * el / steps
    dom = max(kms, key=lambda k: np.mean(kms[k]))
    dom_ms = float(np.mean(kms[dom]))
    # algorithmic bytes of the dominant kernel.  velocity_sums_kernel: velocities (12 B per step) + two sums per
    # trajectory; sample_cost_kernel: every trajectory point once (8 B) + cost out + segment, plus the
    # velocities when it forms the sums itself (option velocity_group = 1 / small batches)
    vel_bytes = 12 * N * (P - 1)
    if dom == "velocity_sums_kernel":
        bytes_launch = vel_bytes + 8 * N
    else:
        bytes_launch = 8 * N * P + 4 * N + 16 * S + (0 if "velocity_sums_kernel" in kms else vel_bytes)
    out = {
        "metric": "CostEvaluator_5k_Trajs (reference benchmark suite), ms per getMinTrajectoryCost",
        "value": ms, "unit": "ms", "n_gpus": 1, "steps": steps, "warmup": warm, "ms_per_step": ms,
        "higher_is_better": False, "scaling": "weak", "vs_baseline": ms / 8.23,
        "vs_baseline_note": "8.23 ms = best published figure for this workload (AMD Strix Halo iGPU through "
                            "AdaptiveCpp, docs/benchmark_log_light.png; other hardware, context only)",
        "dtype": "f32 costs (f64 accumulation as in the reference)", "data": "synthetic",
        "config": {"workload": f"benchmark_runner.cpp:152-185: {N} trajectories x {P} points with velocity profiles, "
                               f"{S}-point tracked segment, weights path=goal=smoothness=jerk=1, samples resident in HBM"},
        "trajectory_points_per_s": N * P / (el / steps),
        "latency_p50_ms": float(np.percentile(np.array(lat) * 1e3, 50)),
        "pcie_inclusive_ms": 1e3 * el_pcie,
        "kernels_ms": {k: float(np.mean(v)) for k, v in kms.items()},
        "roofline": {"bound": "hbm", "kernel": dom, "achieved": bytes_launch / (dom_ms * 1e-3) / 1e9,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": bytes_launch / (dom_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                     "traffic": None, "algorithmic_bytes_per_launch": bytes_launch, "avg_launch_ms": dom_ms,
                     "note": "not an HBM-bound path: the smoothness / jerk sums are serial f64 chains (9 dependent "
                             "instructions per step, velocity_sums_kernel: 4 samples per wavefront), the segment search "
                             "is VALU-issue bound (5.0e9 point x segment-point pairs per call before pruning)"},
        "winner": {"found": bool(r.found), "index": int(r.index), "cost": float(r.cost)},
    }
    if not args.no_cpu:
        ci = ko.CostInputs(w["seg"], w["s0"], w["acc"], w["total"], None, np.float32(10.0) / np.float32(3.0),
                           w["acc_limits"], ko.make_weights(*w["weights"]))
        ncores = usable_cpus()
        t2 = time.perf_counter()
        oi, oc, ocosts = ko.costs_mt(ci, w["px"], w["py"], w["vel"], threads=ncores)
        t_mt = time.perf_counter() - t2
        sub = slice(0, N, max(1, int(np.ceil(t_mt * ncores / max(args.cpu_seconds, 1.0)))))
        t3 = time.perf_counter()
        ko.costs_mt(ci, w["px"][sub], w["py"][sub], [v[sub] for v in w["vel"]], threads=1)
        t_1 = time.perf_counter() - t3
        n_sub = len(range(*sub.indices(N)))
        out["cpu_baseline"] = {
            "value": 1e3 * t_1 * N / n_sub, "unit": "ms", "cores": 1, "kind": "port",
            "sample": f"{n_sub} of the {N} trajectories (every {sub.step}th) on 1 thread: {t_1:.2f} s, scaled to {N}",
            "all_cores": {"value": 1e3 * t_mt, "unit": "ms", "cores": ncores, "sample": "the full workload once"},
            "every_cost_bit_equal": bool(np.array_equal(costs.view(np.uint32), ocosts.view(np.uint32))),
            "gpu_matches_cpu_winner": bool(oi == r.index and np.float32(oc) == np.float32(r.cost)),
        }
    ctx.close()
    return out


def ref_mapper400_bench(args):
    """`--ref mapper400`: Mapper_Dense_400x400 of the reference's benchmark suite
    (benchmark_runner.cpp:190-217): 3600 beams, ranges 5 + 2 sin(20 a), 400x400 @ 0.05."""
    import kompass_hip as kh
    import synthetic as syn
    from oracle import ko

    g = syn.REF_MAPPER400
    H, W, res, n = g["height"], g["width"], g["res"], g["beams"]
    ang, rng = syn.dense_scan(n, 1.0)
    m = kh.MapperContext(H, W, res, (0, 0, 0), 0.0, n)
    for _ in range(args.warmup):
        m.scan_to_grid_device(ang, rng)
        m.sync()
    lat = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ts = time.perf_counter()
        m.scan_to_grid_device(ang, rng)
        m.sync()
        lat.append(time.perf_counter() - ts)
    el = time.perf_counter() - t0
    m.timing_enable(True)
    kms = {}
    for _ in range(min(args.steps, 200)):
        m.scan_to_grid_device(ang, rng)
        m.sync()
        for k, v in m.timings():
            kms.setdefault(k, []).append(v)
    m.timing_enable(False)
    t1 = time.perf_counter()
    for _ in range(50):
        got = m.scan_to_grid(ang, rng)
    el_host = (time.perf_counter() - t1) / 50
    t2 = time.perf_counter()
    want = ko.scan_to_grid(H, W, res, (0, 0, 0), 0.0, ang, rng)
    t_cpu = time.perf_counter() - t2
    ms = 1e3 * el / args.steps
    ray_cells = int((want >= 0).sum())
    bytes_scan = 4 * H * W + 12 * n + 12 * ray_cells
    dom = max(kms, key=lambda k: np.mean(kms[k]))
    dom_ms = float(np.mean(kms[dom]))
    return {
        "metric": "Mapper_Dense_400x400 (reference benchmark suite), ms per scanToGrid", "value": ms, "unit": "ms",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": False,
        "scaling": "weak", "vs_baseline": ms / 0.07,
        "vs_baseline_note": "0.07 ms = best published figure (AMD Strix Halo iGPU, the reference's SYCL mapper -- a "
                            "different algorithm: DDA, rays cut at max_points_per_line; other hardware, context only)",
        "dtype": "int32 grid / f32 endpoints", "data": "synthetic",
        "config": {"workload": f"benchmark_runner.cpp:190-217: {n} beams -> {H}x{W}@{res} grid, CPU-mapper semantics "
                               f"(super-cover Bresenham, ordered stamping), grid resident on the device"},
        "latency_p50_ms": float(np.percentile(np.array(lat) * 1e3, 50)),
        "pcie_inclusive_ms": 1e3 * el_host,
        "kernels_ms": {k: float(np.mean(v)) for k, v in kms.items()},
        "roofline": {"bound": "hbm", "kernel": dom, "achieved": bytes_scan / (dom_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": bytes_scan / (dom_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None,
                     "algorithmic_bytes_per_launch": bytes_scan, "avg_launch_ms": dom_ms},
        "cpu_baseline": {"value": 1e3 * t_cpu, "unit": "ms", "cores": 1, "kind": "port", "sample": "1 scan",
                         "grid_matches": bool(np.array_equal(got, want))},
    }


def hip_library_loaded():
    """True when this process has mapped libkompass_hip.so or the HIP runtime."""
    try:
        maps = open("/proc/self/maps").read()
    except OSError:
        return None
    return ("libkompass_hip" in maps) or ("libamdhip64" in maps)


def launch_ranks(n):
    """`python bench.py --gpus N` without a launcher: N fresh rank processes (torch.distributed.run,
    rendezvous on 127.0.0.1) as CHILDREN of this process, which has not touched the GPU and never will;
    rank 0's JSON line is relayed, the launcher's return code is this script's."""
    import signal
    import socket
    import subprocess

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve())] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC (RCCL across processes on this pool)
    env.setdefault("OMP_NUM_THREADS", "4")
    # The ranks run in a process group of their own with a wall-clock limit: a rank that dies AFTER the
    # rendezvous leaves its peers inside a collective that never completes -- the limit ends the whole group
    # (fresh children only: nothing here re-executes a process that has touched the GPU) and the launcher
    # returns non-zero instead of hanging the caller.
    limit = float(os.environ.get("KC_BENCH_LAUNCH_LIMIT_S", "900"))
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, start_new_session=True)
    timed_out = False
    try:
        stdout, _ = p.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        timed_out = True
        for sig in (signal.SIGTERM, signal.SIGKILL):
            try:
                os.killpg(p.pid, sig)  # the group of the launcher we started, by its exact id
            except ProcessLookupError:
                break
            try:
                p.wait(timeout=10)
                break
            except subprocess.TimeoutExpired:
                continue
        stdout = ""
        try:
            stdout = p.communicate(timeout=5)[0] or ""
        except Exception:  # noqa: BLE001  (pipes of a killed group)
            pass
    line = None
    for ln in (stdout or "").splitlines():
        if ln.startswith("{") and ln.rstrip().endswith("}"):
            line = ln
    rc = p.returncode if p.returncode is not None else 1
    print(f"[bench] launcher pid {os.getpid()}: {n} ranks, rc {rc}{' (wall-clock limit: group terminated)' if timed_out else ''}, "
          f"launcher_loaded_hip_library={hip_library_loaded()}", file=sys.stderr, flush=True)
    if timed_out:
        print(f"[bench] the ranks did not finish within {limit:.0f} s", file=sys.stderr)
        return 124
    if line is not None:
        print(line, flush=True)
    elif rc == 0:
        print("[bench] the ranks printed no JSON line", file=sys.stderr)
        return 1
    return rc


def dry_rank(args, rank, world, local_rank):
    """--dry-launch: what a rank would start from -- no GPU work (launcher test on CPU)."""
    import torch.distributed as dist

    if args.dry_fail_rank == rank:
        sys.exit(3)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    if args.dry_die_after_rendezvous == rank:
        os._exit(5)  # (no clean-up: the peers are left inside the next collective)
    if args.dry_die_after_rendezvous >= 0:
        time.sleep(3600)  # a peer that would wait for ever: only the launcher's limit ends it
    me = {"rank": rank, "local_rank": local_rank, "world": world, "pid": os.getpid(), "ppid": os.getppid(),
          "master": os.environ.get("MASTER_ADDR"), "hip_library_loaded": hip_library_loaded()}
    out = [None] * world
    dist.all_gather_object(out, me)
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"dry_launch": True, "n_gpus": args.gpus, "ranks": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: a timed region of ~0.1 s, so that one scheduling hiccup of the (shared, CPU-quota'd)
    # host -- a few ms -- does not move the mean by tens of percent
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--config", default="cfg2", choices=["cfg1", "cfg2", "cfg3", "cfg5"])
    ap.add_argument("--scene", default="survey", choices=["survey", "mid", "open"],
                    help="costmap of the headline line (SURVEY 8d's by default); the other two follow in the same JSON")
    ap.add_argument("--split", action="store_true", help="three-kernel cycle instead of the single launch")
    ap.add_argument("--fresh", action="store_true",
                    help="only the fresh_inputs leg (one reference cycle per step), as the top-level line (profiling passes)")
    ap.add_argument("--scan", action="store_true",
                    help="only the laserscan_room leg (LaserScan input, 1440 beams), as the top-level line (profiling passes)")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: per-kernel times and roofline, the CPU baseline and the other legs "
                         "(scenes, LaserScan, input updates, fresh inputs, mapper; with several ranks the strong-scaling block)")
    ap.add_argument("--only-headline", action="store_true",
                    help="with --full: no mid_density / open_space / extras legs (profiling passes: one scene per process)")
    ap.add_argument("--mapper", action="store_true", help="bench the LocalMapper (cfg4) instead")
    ap.add_argument("--bayes", action="store_true", help="with --mapper: the Bayesian mapping loop (8f rank 3)")
    ap.add_argument("--pointcloud", action="store_true", help="SURVEY 8f rank 1 instead of the controller")
    ap.add_argument("--ref", choices=["cost5k", "mapper400"],
                    help="the reference's own published benchmark workloads (benchmark_runner.cpp) instead")
    ap.add_argument("--dry-launch", action="store_true",
                    help="start the ranks, report their environment, do no GPU work (launcher test)")
    ap.add_argument("--dry-fail-rank", type=int, default=-1, help="with --dry-launch: this rank exits with code 3")
    ap.add_argument("--dry-die-after-rendezvous", type=int, default=-1,
                    help="with --dry-launch: this rank dies behind the rendezvous, its peers wait for ever (launcher limit test)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the cpu_baseline leg")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the timed cycle returned in its last step as DIR/<name>.npy (controller lines only)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and (args.mapper or args.pointcloud or args.ref or args.dry_launch):
        ap.error("--dump-outputs covers the controller lines (the default, --fresh, --scan)")
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus))
    if args.dry_launch:
        return dry_rank(args, rank, world, local_rank)
    # stdout carries exactly ONE JSON line: native libraries (RCCL prints a version
    # banner on stdout when the first communicator comes up) are pointed at stderr
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    try:
        out = (ref_cost5k_bench(args) if args.ref == "cost5k" else ref_mapper400_bench(args) if args.ref == "mapper400" else
               bayes_mapper_bench(args) if args.mapper and args.bayes else
               mapper_bench(args) if args.mapper else pointcloud_bench(args) if args.pointcloud
               else controller_bench(args, rank, world, local_rank))
    finally:
        sys.stdout.flush()
        os.dup2(real_stdout, 1)
        os.close(real_stdout)
    if rank == 0 and out is not None:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
