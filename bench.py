#!/usr/bin/env python3
"""bench.py -- headline benchmark of the seed-and-extend hot path on MI355X.

Workload (BASELINE.json configs[1]): batched banded Smith-Waterman/Gotoh, 10 M x 100 bp
reads vs 150 bp reference windows per GPU, band 15, LOCAL, scheme (2,-1,-2,-1); inputs are
generated on the device and are resident in HBM before the timed region.  A "step" is one
pass of the extension kernel over the whole batch (for N>1: over every rank's shard, plus the
gather of the result records to rank 0 over RCCL/xGMI, overlapped with the next step).

A plain run sets up, warms up, times the steps and prints the result line (the last stdout line);
`--dump-outputs DIR` also writes what the last timed step computed (benchlib/dump.py).  With
`--full` the same run also checks a sample against the CPU oracle (`parity`), times the all-int32
kernel (`roofline.a32`) and runs the other legs (not part of `value`): the FM-index rank()
point-query kernel on a 3 Gbp-sized index (the second half of BASELINE.json's metric), reported as
`rank_roofline`, the seed / end-to-end / full-matrix / drop-in stream legs, and the CPU oracle timed
on the host cores (`cpu_baseline`); every leg also goes to the legs file.

  python bench.py --gpus 1 --steps 20 --warmup 3
  python bench.py --gpus 1 --steps 20 --warmup 3 --full
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist

import nvbio_amd as nvb
from nvbio_amd import workloads as W
from nvbio_amd.distributed import ResultGather

# MI355X peaks (/opt/skills/guides/MI355X_MICROARCH.md)
HBM_PEAK_GBS = 8000.0
VALU_PEAK_TOPS = 256 * 4 * 32 * 2.4e9 / 1e12      # int32 lane-ops/s: 256 CU x 4 SIMD-32 x 2.4 GHz = 78.6 T

READ_LEN, REF_LEN, BAND = 100, 150, 15
SCHEME = (2, -1, -2, -1)
# algorithmic figures per alignment
CELLS_PER_ALN = READ_LEN * BAND                    # 1500 band cells
NOMINAL_OPS_PER_CELL = 14                          # reference recurrence, int ops per cell (LOCAL, the headline's type)
FULL_NOMINAL_OPS_PER_CELL = {"local": 14, "semi_global": 12, "global": 11}   # the same recurrence per alignment type
BYTES_PER_ALN = 50 + 29 + 12 + 8                   # packed read + text window + sink record + offsets = 99 B
RANK_BYTES_PER_QUERY = 40                          # 32 B record + 4 B query + 4 B result


def measured_counter(kernel, key):
    """Another per-launch counter of the same PMC passes (profiles/traffic.json), None if absent."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            return json.load(f).get(kernel, {}).get(key)
    except Exception:
        return None


def dp_counters(kernel):
    """The two DP-path counters north_star names -- L2 hit rate and LDS bank conflicts -- from the committed PMC passes of this command
    (profiles/traffic.json, taken on the round's final code): TCC_HIT_sum / (TCC_HIT_sum + TCC_MISS_sum); SQ_LDS_BANK_CONFLICT (extra cycles)
    over SQ_LDS_IDX_ACTIVE (all LDS-array cycles).  None if the pass is absent."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            pm = json.load(f).get(kernel, {})
    except Exception:
        return None
    if pm.get("l2_hit") is None or pm.get("lds_idx_active_cycles") is None:
        return None
    return {"l2_hit": pm["l2_hit"], "l2_miss": pm["l2_miss"], "l2_hit_rate": pm["l2_hit"] / max(pm["l2_hit"] + pm["l2_miss"], 1),
            "lds_bank_conflict_cycles": pm["lds_bank_conflict_cycles"], "lds_active_cycles": pm["lds_idx_active_cycles"],
            "lds_bank_conflict_frac": pm["lds_bank_conflict_cycles"] / max(pm["lds_idx_active_cycles"], 1),
            "source": pm.get("counters_source")}


def physical_cores():
    """Physical cores of the host (distinct (package, core) pairs in /proc/cpuinfo), None if it cannot be read."""
    try:
        pairs, pkg = set(), None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                pkg = line.split(":")[1].strip()
            elif line.startswith("core id"):
                pairs.add((pkg, line.split(":")[1].strip()))
        return len(pairs) or None
    except OSError:
        return None


def counters_round(kernel):
    """which round's PMC pass a replayed counter of profiles/traffic.json was taken in (every entry carries it)"""
    return measured_counter(kernel, "round")


def measured_traffic(kernel):
    """HBM-side bytes per launch from the committed rocprofv3 --pmc passes of this same command
    (profiles/traffic.json: TCC_EA0_RDREQ x request size + TCC_EA0_WRREQ x 64 B); None if absent."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            return json.load(f).get(kernel, {}).get("hbm_bytes_per_launch")
    except Exception:
        return None


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 200: ~0.6 s of timed region)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reads", type=int, default=10_000_000, help="reads per GPU")
    ap.add_argument("--genome", type=float, default=3.0e9, help="synthetic genome length of the FM-index legs (a true index is built on the device)")
    ap.add_argument("--rank-queries", type=int, default=1 << 28)
    ap.add_argument("--no-rank", action="store_true")
    ap.add_argument("--only", choices=["dp", "rank", "seed", "e2e", "full", "extras", "compat", "refapp", "repeats"], default=None, help="profiling aid: run just one leg, print its object")
    ap.add_argument("--seeds", type=int, default=50_000_000)
    ap.add_argument("--pairs", type=int, default=500_000, help="read pairs of the paired-end driver leg inside the e2e leg (0 = skip)")
    ap.add_argument("--share-pairs", type=int, default=25_000_000, help="config 5 at one GPU's share of 200 M pairs over 8 GPUs (0 = skip); runs in batches of --pairs")
    ap.add_argument("--no-seed", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--no-full", action="store_true")
    ap.add_argument("--full-reads", type=int, default=65536)
    ap.add_argument("--full-ref", type=int, default=16384)
    ap.add_argument("--e2e-reads", type=int, default=10_000_000, help="reads per batch of the end-to-end seed+locate+extend leg")
    ap.add_argument("--e2e-batches", type=int, default=5, help="batches of the full-size run of BASELINE config 4 (5 x 10 M = 50 M reads)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--ref-app", action="store_true", help="also run the leg that runs the reference's own nvBowtie binary (oracle/_ref/ref_nvBowtie) at config-4 size: writes 3.75 GB of index files, ~40 s; opt-in")
    ap.add_argument("--no-repeat-rich", action="store_true", help="skip the single-end driver on the repeat-rich 3 Gbp genome (a second genome and index: ~25 s)")
    ap.add_argument("--repeat-rich-reads", type=int, default=5_000_000)
    ap.add_argument("--legs-file", default=None, help="where the full per-leg objects go (default: gpurun_out/bench_legs.json if that directory exists, else ./bench_legs.json)")
    ap.add_argument("--ref-app-reads", type=int, default=5_000_000)
    ap.add_argument("--cpu-sample", type=int, default=10_000_000)
    ap.add_argument("--full", action="store_true", help="also run the oracle parity gate, the all-int32 timing and every other leg (off: the timed steps only)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="write the last timed step's scores and sinks to DIR/*.npy (float64)")
    return ap.parse_args()


def main():
    a = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.steps is None:
        a.steps = 200
    if a.only is not None:
        a.full = True       # --only runs one leg of the full run, as the full run runs it
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("NVBIO_BENCH_SHARE_GPU") == "1":
        local = 0          # debugging aid: all ranks on one GPU (exercises the N>1 control flow on a 1-GPU box)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the hot path has no CPU fallback")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if os.environ.get("NVBIO_BENCH_SHARE_GPU") == "1":
            dist.init_process_group("gloo")       # RCCL refuses two ranks on one device; gloo stages the gather through the host
        else:
            dist.init_process_group("nccl", device_id=dev)
    assert world == a.gpus, "launch with torch.distributed.run --nproc-per-node == --gpus"

    def barrier():
        if world > 1:
            if dist.get_backend() == "nccl":
                dist.barrier(device_ids=[local])
            else:
                dist.barrier()
        torch.cuda.synchronize()

    if a.only == "extras":
        print(json.dumps({"extras_leg": extras_leg(a, dev)}))
        return
    if a.only == "full":
        print(json.dumps({"full_dp_leg": full_dp_leg(a, dev)}))
        return
    if a.only == "compat":
        print(json.dumps({"compat_stream_leg": compat_stream_leg(a, dev)}))
        return
    if a.only in ("rank", "seed", "e2e"):
        a.no_seed = a.only != "seed"
        a.no_rank = a.only != "rank"
        a.no_e2e = a.only != "e2e"
        print(json.dumps(fm_legs(a, dev)))
        return
    if a.only == "repeats":
        print(json.dumps({"repeat_rich": repeat_rich_leg(a, dev)}))
        return
    if a.only == "refapp":
        print(json.dumps({"ref_nvbowtie_leg": ref_nvbowtie_leg(a, dev)}))
        return
    if a.only == "dp":
        a.no_rank = a.no_cpu = a.no_seed = a.no_e2e = a.no_full = a.no_repeat_rich = True; a.ref_app = False

    # ---------------------------------------------------------------- inputs (resident before timing)
    n = a.reads
    patterns, texts = W.make_sw_batch(n, READ_LEN, REF_LEN, seed=0x5EED0002 + rank, device=dev)
    aligner = nvb.make_gotoh_aligner(nvb.LOCAL, nvb.SimpleGotohScheme(*SCHEME))
    batch = nvb.BatchedBandedAlignmentScore(BAND)
    comm_stream = torch.cuda.Stream(device=dev) if world > 1 else None

    def launch(buf):
        batch.enact(aligner, patterns, texts, buf[0], buf[1])

    # result records: score[n] + sink[n,2], gathered as 4 B per read (score:16, sink.x:8, sink.y:8 -- 100 bp reads); double-buffered so that the gather
    # of step k (side stream) overlaps the kernel of step k+1
    outs = [(torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev)) for _ in range(2)]
    gatherers = [ResultGather(n * world, dst=0, device=dev, record_bytes=4) for _ in range(2)] if world > 1 else None

    pending = [None, None]
    # The gather of the result records.  First choice: the C++ path -- RCCL ncclSend / ncclRecv issued through the C-ABI
    # (nvbio_hip_gather_records; include/nvbio_hip/multi_device.h), its communicator opened from a unique id that torch.distributed
    # only ships.  Second choice: torch.distributed.gather.  Every rank tries on tiny buffers first and all agree on the outcome, so a
    # backend that cannot do it is found here -- the run then continues ("gather_path" says how) instead of dying mid-measurement.
    gather_on, gather_path, cxx_comm, cxx_g, ranks_seen = world > 1, None, None, None, 0
    if world > 1:
        from nvbio_amd.distributed import CxxComm, CxxRecordGather, pack_result_records
        on_nccl = dist.get_backend() == "nccl"

        def agree(flag):
            ft = torch.tensor([flag], dtype=torch.int32, device=dev if on_nccl else "cpu")
            dist.all_reduce(ft, op=dist.ReduceOp.MIN)
            return bool(int(ft.item()))

        flag = 1
        try:
            host_transport = os.environ.get("NVBIO_BENCH_HOST_TRANSPORT") == "1"
            if host_transport:
                # the production C++ gather with only ncclSend / ncclRecv replaced (nvbio_hip_comm_set_transport: gloo carries the bytes): what two
                # ranks sharing one device -- where RCCL refuses to open -- can exercise of the N > 1 path (tests/test_bench_multirank_gpu.py)
                from nvbio_amd.distributed import HostTransportComm
                cxx_comm = HostTransportComm()
            elif not on_nccl or os.environ.get("NVBIO_BENCH_TORCH_GATHER") == "1":
                raise RuntimeError("C++ gather needs one device per rank")
            else:
                cxx_comm = CxxComm()
            pg = CxxRecordGather(cxx_comm, world * 4, 1, dst=0, device=dev)
            pg.gather(torch.full((4, 1), rank, dtype=torch.int32, device=dev))
            torch.cuda.synchronize()
            if rank == 0:
                ranks_seen = sum(1 for r in range(world) if bool((pg.shard(r) == r).all()))      # ranks whose probe records arrived intact through the C++ gather
                if ranks_seen != world:
                    raise RuntimeError("C++ gather returned wrong records (%d of %d ranks seen)" % (ranks_seen, world))
        except Exception as e:     # noqa: BLE001
            sys.stderr.write("bench: C++ / RCCL gather unavailable on rank %d (%s); trying torch.distributed\n" % (rank, e))
            flag = 0
        if agree(flag):
            gather_path = ("cxx_host_transport (nvbio_hip_gather_records over a gloo-backed transport table)" if os.environ.get("NVBIO_BENCH_HOST_TRANSPORT") == "1"
                           else "cxx_rccl (nvbio_hip_gather_records: grouped ncclSend/ncclRecv from C++)")
            cxx_g = [CxxRecordGather(cxx_comm, n * world, 1, dst=0, device=dev) for _ in range(2)]
        else:
            cxx_comm = None
            ranks_seen = 0
            flag = 1
            try:
                probe = ResultGather(world * 4, dst=0, device=dev, record_bytes=4)
                probe.gather(torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros((4, 2), dtype=torch.int32, device=dev), concat=False)
                torch.cuda.synchronize()
            except Exception as e:     # noqa: BLE001
                sys.stderr.write("bench: result gather unavailable (%s); continuing without it\n" % e)
                flag = 0
            gather_on = agree(flag)
            gather_path = "torch.distributed.gather" if gather_on else None
    overflow = [None, None]

    def step(i, events=None):
        b = i & 1
        if gather_on and pending[b] is not None:
            torch.cuda.current_stream().wait_event(pending[b])        # gather of step i-2 done: buffer b is free
        if events is not None:
            events[0].record()
        launch(outs[b])
        if events is not None:
            events[1].record()
        if gather_on:
            comm_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(comm_stream):
                if cxx_g is not None:
                    rec, overflow[b] = pack_result_records(outs[b][0], outs[b][1], 4)
                    cxx_g[b].gather(rec, concat=False)                      # 4 B/read to rank 0 over RCCL/xGMI, issued from C++
                else:
                    gatherers[b].gather(outs[b][0], outs[b][1], concat=False)   # ... or through torch.distributed
                pending[b] = torch.cuda.Event()
                pending[b].record(comm_stream)

    # ---------------------------------------------------------------- parity gate (sample vs oracle; --full)
    parity = None
    if rank == 0 and a.full:
        from oracle import pyoracle as O          # checker only
        import numpy as np
        launch(outs[0])
        torch.cuda.synchronize()
        m = min(n, 100_000)
        sub_p = nvb.PackedStringSet(patterns.words, 4, True, patterns.begin[:m].contiguous(), None, READ_LEN)
        sub_t = nvb.PackedStringSet(texts.words, 2, False, texts.begin[:m].contiguous(), None, REF_LEN)
        es, ek = O.batch_banded_gotoh_score(BAND, O.LOCAL, SCHEME, O.StringSet.from_device(sub_p), O.StringSet.from_device(sub_t))
        ok = bool((outs[0][0][:m].cpu().numpy() == es).all() and (outs[0][1][:m].cpu().numpy().view(np.uint32) == ek).all())
        parity = {"checked": m, "bit_exact": ok}
        if not ok:
            raise SystemExit("parity gate failed: HIP scores differ from the oracle")

    # ---------------------------------------------------------------- timed region
    for i in range(a.warmup):
        step(i)
    barrier()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
    t0 = time.perf_counter()
    for i in range(a.steps):
        step(i, evs[i])
    if world > 1:
        torch.cuda.current_stream().wait_stream(comm_stream)
    barrier()
    t1 = time.perf_counter()
    elapsed = t1 - t0
    per_rank_ms = None
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
        every = [torch.zeros_like(tt) for _ in range(world)]
        dist.all_gather(every, tt)                                   # each rank's own clock, for the line; the job's time is their maximum
        per_rank_ms = [float(x.item()) / a.steps * 1e3 for x in every]
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    kern_ms = sum(e0.elapsed_time(e1) for e0, e1 in evs) / max(a.steps, 1)
    if rank == 0 and a.dump_outputs and a.steps > 0:
        from benchlib import dump
        dump.write_outputs(a.dump_outputs, *outs[(a.steps - 1) & 1])
    # the same launch on the all-int32 kernel (what runs when the host cannot prove the 16-bit form exact; --full)
    a32_ms = None
    if rank == 0 and world == 1 and a.full:
        nvb.set_test_switch("NVBIO_HIP_FORCE_32BIT", "1")
        launch(outs[1]); torch.cuda.synchronize()
        ev32 = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(5)]
        for e0, e1 in ev32:
            e0.record(); launch(outs[1]); e1.record()
        torch.cuda.synchronize()
        nvb.set_test_switch("NVBIO_HIP_FORCE_32BIT", 0)
        a32_ms = sum(e0.elapsed_time(e1) for e0, e1 in ev32) / len(ev32)
        a32_same = bool(torch.equal(outs[1][0], outs[0][0]) and torch.equal(outs[1][1], outs[0][1]))
    if gather_on and cxx_g is not None:
        if any(o is not None and bool(o.item()) for o in overflow):
            raise SystemExit("result gather: records did not fit the 4-byte format")
    elif gather_on and rank == 0 and any(g.overflowed() for g in gatherers):
        raise SystemExit("result gather: records did not fit the 4-byte format")

    out = None
    if rank == 0:
        total_reads = n * world * a.steps
        value = total_reads / elapsed
        kt = kern_ms * 1e-3
        roofline = {
            "kernel": "banded_gotoh_score_kernel<15,LOCAL>",
            "bound": "valu",
            "achieved": n * CELLS_PER_ALN * NOMINAL_OPS_PER_CELL / kt / 1e12,
            "peak": VALU_PEAK_TOPS,
            "unit": "Tint-op/s",
            "frac": n * CELLS_PER_ALN * NOMINAL_OPS_PER_CELL / kt / 1e12 / VALU_PEAK_TOPS,
            "traffic": measured_traffic("banded_gotoh_score_kernel"),
            "traffic_round": counters_round("banded_gotoh_score_kernel"),      # the round whose PMC pass the replayed counters come from
            "kernel_ms": kern_ms,
            "gcups": n * CELLS_PER_ALN / kt / 1e9,
            "hbm_GBs": n * BYTES_PER_ALN / kt / 1e9,
            "hbm_frac": n * BYTES_PER_ALN / kt / 1e9 / HBM_PEAK_GBS,
            "note": "integer DP: neither HBM nor MFMA binds it; peak = VALU lane-ops/s at 32 lanes/clk (the rate of the 16-bit ops the kernel is built from), achieved = cells x 14 nominal ops (SURVEY 8d: the reference recurrence's count); since the row-frame cell of round 6 the kernel ISSUES fewer (11 instructions per LOCAL cell + the row's set-up: `executed`), so `frac` -- the reference's operations per second over the instruction peak -- can touch 1, and `executed.frac` is the VALU issue utilisation; results are the reference's int32 scores, computed in int16 where provably exact",
        }
        # executed instructions (SQ_INSTS_VALU of the committed PMC pass, wave instructions x 64 lanes) next to the nominal-op count
        iv = measured_counter("banded_gotoh_score_kernel", "insts_valu_per_launch")
        if iv is not None:
            iv_reads = measured_counter("banded_gotoh_score_kernel", "insts_valu_reads") or n
            roofline["executed"] = {"valu_lane_ops_per_cell": iv * 64.0 / iv_reads / CELLS_PER_ALN, "nominal_ops_per_cell": NOMINAL_OPS_PER_CELL,
                                    "achieved": iv / iv_reads * n * 64 / kt / 1e12, "unit": "T lane-op/s",
                                    "frac": iv / iv_reads * n * 64 / kt / 1e12 / VALU_PEAK_TOPS, "source": "SQ_INSTS_VALU, profiles/traffic.json"}
        roofline["counters"] = dp_counters("banded_gotoh_score_kernel")
        if a32_ms is not None:
            roofline["a32"] = {"kernel": "banded_gotoh_score_kernel<15,LOCAL,A32>", "kernel_ms": a32_ms, "gcups": n * CELLS_PER_ALN / (a32_ms * 1e-3) / 1e9,
                               "reads_per_s": n / (a32_ms * 1e-3), "frac": n * CELLS_PER_ALN * NOMINAL_OPS_PER_CELL / (a32_ms * 1e-3) / 1e12 / VALU_PEAK_TOPS,
                               "identical_results": a32_same}
        out = {
            "metric": "aligned reads/s (100 bp, band=15)", "value": value, "unit": "reads/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": elapsed / a.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "int16", "data": "synthetic",
            "config": {"workload": "nvbio::aln batched banded SW (configs[1]): %d x 100 bp reads vs 150 bp windows per GPU, band=15, LOCAL Gotoh (2,-1,-2,-1)" % n,
                       "reads_per_gpu": n, "read_len": READ_LEN, "band": BAND, "type": "LOCAL", "parallelism": "read-shard x%d, gather to rank 0" % world, "gather": bool(gather_on) if world > 1 else None, "gather_path": gather_path,
                       "rccl_ranks_seen": ranks_seen if world > 1 else None, "per_rank_ms_per_step": per_rank_ms},
            "roofline": roofline, "parity": parity,
        }

    # ---------------------------------------------------------------- FM-index rank leg and the other legs (rank 0, N == 1 only; --full)
    if rank == 0 and world == 1 and a.full and not (a.no_rank and a.no_seed and a.no_e2e):
        del patterns, texts, outs
        torch.cuda.empty_cache()
        out.update(fm_legs(a, dev))
    if rank == 0 and world == 1 and a.full and not a.no_full:
        out["full_dp_leg"] = full_dp_leg(a, dev)
        out["compat_stream_leg"] = compat_stream_leg(a, dev)
    if rank == 0 and world == 1 and a.full and not a.no_e2e and not a.no_repeat_rich:
        torch.cuda.empty_cache()
        nvb.lib().nvbio_hip_device_trim()
        out.setdefault("e2e_leg", {})["repeat_rich"] = repeat_rich_leg(a, dev)
    if rank == 0 and world == 1 and a.full and a.ref_app:
        torch.cuda.empty_cache()
        out["ref_nvbowtie_leg"] = ref_nvbowtie_leg(a, dev)
    if rank == 0 and world == 1 and a.full and not a.no_cpu:
        out["cpu_baseline"] = cpu_leg(a, *W.make_sw_batch(min(n, a.cpu_sample), READ_LEN, REF_LEN, seed=0x5EED0002, device=dev))
    # ---------------------------------------------------------------- nvBowtie end to end, sharded (N > 1): BASELINE config 4's "1 vs 8 GPU shard"
    if world > 1 and a.full and not a.no_e2e:
        del patterns, texts, outs
        torch.cuda.empty_cache()
        leg = e2e_sharded_leg(a, dev, rank, world, barrier, cxx_comm)
        if rank == 0:
            out["e2e_sharded_leg"] = leg
    if rank == 0:
        if a.full:
            emit(out, a.legs_file)
        else:
            from benchlib import headline as H
            print(H.headline_line(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


def emit(out, legs_file=None):
    """Every leg on its own stdout line and in the legs file; then the compact headline (benchlib/headline.py: < 4 KB, the contract's keys
    + roofline + rank_roofline + cpu_baseline + parity) as the LAST line -- the one the driver parses."""
    from benchlib import headline as H
    if legs_file is None:
        d = os.path.join(ROOT, "gpurun_out")
        legs_file = os.path.join(d, "bench_legs.json") if os.path.isdir(d) else os.path.join(os.getcwd(), "bench_legs.json")
    try:
        with open(legs_file, "w") as f:
            json.dump(out, f, indent=1)
        shown = os.path.relpath(legs_file, ROOT) if legs_file.startswith(ROOT) else legs_file
    except OSError as e:
        sys.stderr.write("bench: could not write %s (%s)\n" % (legs_file, e))
        shown = None
    for line in H.leg_lines(out):
        print(line)
    print(H.headline_line(out, shown), flush=True)


def repeat_rich_leg(a, dev):
    """BASELINE config 4 on a genome that looks like one: the repeat-rich 3 Gbp genome of tools/nvbowtie_3gbp.py (60 % of it diverged copies of three
    repeat families, the largest with three million copies) -- the genome on which every SAM record of this driver is held to the unchanged
    nvBowtie's (tests/test_ref_tests_gpu.py) -- through the C++ single-end driver in nvBowtie's own batches of 1024 K reads (the hits-per-read
    rule of both drivers reasons with the batch), on the index the loaders build by default (FMIndexDevice.hbm_default), one batch at a time
    and two in flight; every batch's (best, mapq) compared with the same driver on the reference-layout index.  Where a batch's time goes:
    `one_batch.stage_ms_with_syncs`; the i.i.d. genome of `config4_full_size` takes 8-10 extension rounds per batch, this one 113."""
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import own_driver_3gbp as T
        r = T.measure(int(a.genome), a.repeat_rich_reads, 1 << 20, 0.6, "default", (1, 2), check=False, stage_clock=True, reps=2, lean_check=True)
    except Exception as e:      # noqa: BLE001
        return {"error": repr(e)[:500]}
    return {"genome": r["genome"], "repeats": r["repeats"], "repeat_families": r["repeat_families"], "reads": r["reads_aligned"], "batch_reads": r["batch"], "driver": r["driver"],
            "index": r["index_built"], "one_batch": r.get("one_batch"), "serial": r["pipelined"].get("1"), "two_batches_in_flight": r["pipelined"].get("2"),
            "Mreads_per_s": r["Mreads_per_s"], "rounds": (r.get("one_batch") or {}).get("rounds"), "extensions": (r.get("one_batch") or {}).get("extensions"),
            "identical_to_reference_layout": r.get("identical_to_reference_layout"),
            "identical_to_reference_driver": "every SAM record of this driver on this genome equals the unchanged nvBowtie's: tests/test_ref_tests_gpu.py::test_reference_nvbowtie_equals_own_driver_at_3gbp (python bench.py --ref-app reruns it here)"}


def ref_nvbowtie_leg(a, dev):
    """BASELINE config 4 through the REFERENCE'S OWN APPLICATION: nvBowtie's 29 translation units compiled as they lie on the drop-in layer and linked
    with libnvbio_hip.so (oracle/_ref/ref_nvBowtie, built where /root/reference exists) -- a caller of the product, not a checker -- on a 3 Gbp
    repeat-rich synthetic genome written as .bwt/.sa/.rbwt/.rsa/.wpac/.ann/.amb and a FASTQ file, beside this repository's driver on the same files
    (tools/nvbowtie_3gbp.py).  Reports nvBowtie's own per-stage device seconds and whether every SAM record of the two is identical."""
    import re
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_nvBowtie")
    if not os.path.exists(exe):
        return {"skipped": "oracle/_ref/ref_nvBowtie is not built (needs /root/reference in the build container)"}
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import nvbowtie_3gbp as T
        res, log = T.run(int(a.genome), a.ref_app_reads, 0.6)
    except Exception as e:      # noqa: BLE001
        return {"error": repr(e)[:500]}
    stages = {}
    for name, secs, dev_s in re.findall(r"stats\s+: \[0\]\s+(\w[\w ]*?)\s+: ([0-9.]+) sec \(.*?([0-9.]+) device sec\)", log.replace("\r", "\n")):
        stages[name.strip()] = {"wall_s": float(secs), "device_ms": float(dev_s) * 1e3}
    total = re.findall(r"stats\s+: \[0\]\s+total\s+: ([0-9.]+) sec", log)
    out = {"genome": res.get("genome"), "repeats": res.get("repeats"), "reads": res.get("reads"), "index_files_GB": res.get("index_files_GB"),
           "nvbowtie": {"exit": res.get("nvbowtie_exit"), "wall_s_incl_index_load_and_io": res.get("nvbowtie_wall_s"),
                        "align_s": float(total[0]) if total else None, "reads_per_s": (res.get("reads") / float(total[0])) if total else None,
                        "stages": stages, "line_native_records": os.environ.get("NVBIO_HIP_COMPAT_LINE_NATIVE", "1") != "0"},
           "own_driver": {"align_s": res.get("own_align_s"), "reads_per_s": res.get("own_reads_per_s"), "batches": res.get("own_batches"), "sam_write_s": res.get("own_write_s")},
           "records": res.get("records_ref"), "identical_records": res.get("identical"), "difference_categories": res.get("difference_categories"),
           "every_record_identical": res.get("identical") is not None and res.get("identical") == res.get("records_ref") == res.get("records_own")}
    return out


def e2e_sharded_leg(a, dev, rank, world, barrier, cxx_comm=None):
    """nvBowtie's single-end driver (nvbio_amd.aligner.best_approx) with the read batch sharded across the ranks: every GPU holds the
    whole index (built from the same seed) and aligns its own e2e_reads reads; no collective inside the pipeline.  Timed like the
    headline: barrier + synchronize on both sides, maximum over ranks.  Ranks first agree that set-up and a warm-up run succeeded
    everywhere, so that a local failure cannot leave the others waiting in the timed region."""
    from nvbio_amd import aligner as AL, select as SEL, pipeline as P
    from nvbio_amd.distributed import RecordGather, CxxRecordGather, alignment_records
    cpu = dist.get_backend() != "nccl"
    state, err = {}, ""
    try:
        ng, n = int(a.genome), a.e2e_reads
        g = torch.Generator(device=dev)
        g.manual_seed(0x5EED0003)
        text = torch.randint(0, 4, (ng,), dtype=torch.uint8, generator=g, device=dev)
        genome_words = W._pack_chunked(text, 2, True)
        sym, pos, _ = P.make_reads(text, n, READ_LEN, seed=0x5EED0004 + rank)
        fmi, index_desc = hbm_rich(W.build_fm_index(text), dev)     # every rank its own copy: two-symbol arrays + k-mer table + full SA as memory allows
        state["index"] = index_desc
        del text
        packed = P.pack_read_streams(sym)
        names = SEL.pack_names(["r%d.%d" % (rank, i) for i in range(n)], dev)
        prm = AL.Params(hits_stride=16, batch_size=n)
        # 16 B per read to rank 0: alignment word, position, MAPQ, read id -- from C++ over RCCL when the pre-flight found it
        gat = CxxRecordGather(cxx_comm, n * world, 4, dst=0, device=dev) if cxx_comm is not None else RecordGather(n * world, 4, dst=0, device=dev)
        def align():
            return AL.best_approx(fmi, None, sym, genome_words, ng, prm, names=names, packed=packed)
        def run():
            r = align()
            r["table"] = gat.gather(alignment_records(r["best"][0], r["mapq"], rank * n), concat=False)
            return r
        align(); torch.cuda.synchronize()          # local warm-up only: the gather is a collective and waits for the agreement below
        state.update(run=run, n=n, ng=ng, pos=pos, gat=gat)
    except Exception as e:          # noqa: BLE001 -- reported, and agreed on below
        err = "%s: %s" % (type(e).__name__, e)
    ok = torch.tensor([0 if err else 1], dtype=torch.int32, device="cpu" if cpu else dev)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if int(ok.item()) == 0:
        return {"error": err or "another rank failed during set-up"}
    state["run"](); torch.cuda.synchronize()       # warm-up of the whole step, gather included: every rank is here
    barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = state["run"]()
    torch.cuda.synchronize(); barrier()
    elapsed = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device="cpu" if cpu else dev)
    dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    loc = (r["best"][0] >> 32) & 0xFFFFFFFF
    aligned = loc != 0xFFFFFFFF
    frac = torch.tensor([float(aligned.float().mean().item()), float((aligned & ((loc - state["pos"]).abs() <= 2)).float().mean().item())],
                        dtype=torch.float64, device="cpu" if cpu else dev)
    dist.all_reduce(frac, op=dist.ReduceOp.SUM)
    n, el = state["n"], float(elapsed.item())
    gathered_ok = None
    if rank == 0:
        # the root's receive buffers hold every rank's records in rank order: its own shard must equal what it sent, and
        # the read ids of the other shards must be theirs
        gat = state["gat"]
        own = alignment_records(r["best"][0], r["mapq"], 0)
        part = (lambda k: gat.shard(k)) if cxx_comm is not None else (lambda k: gat.bufs[k][:n])
        gathered_ok = bool(torch.equal(part(0), own)) and all(
            bool((part(k)[:, 3] == torch.arange(k * n, (k + 1) * n, device=dev, dtype=torch.int64).to(torch.int32)).all()) for k in range(1, world))
    return {"driver": "nvbio_amd.aligner.best_approx (Aligner::best_approx: seeding passes, randomized selection, band-31 extension, reduce, MAPQ, traceback)",
            "index": state.get("index"), "gather": True, "gather_path": "cxx_rccl" if cxx_comm is not None else "torch.distributed.gather", "gather_record_bytes": 16, "gathered_records_verified": gathered_ok,
            "genome_symbols": state["ng"], "reads_per_gpu": n, "n_gpus": world, "ms_per_batch": el * 1e3, "Mreads_per_s": n * world / el / 1e6,
            "aligned": float(frac[0].item()) / world, "best_at_true_position": float(frac[1].item()) / world,
            "sharding": "reads block-sharded, index replicated, no collective inside the pipeline; one gather of 16-byte alignment records to rank 0 per batch, inside the timed region"}


def fm_legs(a, dev):
    """The FM-index half of the metric on ONE true index of a synthetic i.i.d. genome (BASELINE
    config 3: 3 Gbp), built on the device: rank() point queries (`rank_roofline`) and
    match + locate of 22-bp seeds (`seed_leg`)."""
    ng = int(a.genome)
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED0003)
    text = torch.randint(0, 4, (ng,), dtype=torch.uint8, generator=g, device=dev)
    t0 = time.perf_counter()
    fmi = W.build_fm_index(text)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    out = {}
    if not a.no_rank:
        out["rank_roofline"] = rank_leg(a, dev, fmi)
    if not a.no_seed:
        out["seed_leg"] = seed_leg(a, dev, fmi, text, build_s)
    if not a.no_e2e:
        out["e2e_leg"] = e2e_leg(a, dev, fmi, text)
    return out


def e2e_leg(a, dev, fmi, text):
    """BASELINE config 4's shape: single-end 100-bp reads against the 3 Gbp index through the composed
    driver nvbio_amd.pipeline (map_exact -> locate -> banded extend, band 15, -> best per read).  The
    select / reduce glue between the kernels is torch tensor code, not nvBowtie's policy; a sample is
    checked exactly against the same glue over the oracle."""
    import numpy as np
    from nvbio_amd import pipeline as P
    from oracle import pyoracle as O
    ng, n = fmi.length, a.e2e_reads
    genome_words = W._pack_chunked(text, 2, True)
    sym, pos, _ = P.make_reads(text, n, READ_LEN, seed=0x5EED0004)
    mp = nvb.MappingParams()
    packed = P.pack_read_streams(sym)                  # inputs resident in HBM before the timed region
    res = {}
    for name, idx in (("reference_layout", fmi), ("line_native", "dimer"), ("hbm_rich_ktab12_ssa1", None)):
        if idx is None:
            idx = fmi.with_ktab(12).with_dense_ssa(1)
        elif idx == "dimer":
            idx = fmi.with_dimer()
        be = P.HipBackend(idx, None, mp, READ_LEN)
        P.seed_and_extend(be, sym, genome_words, ng, packed=packed)        # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        score, bpos, n_jobs = P.seed_and_extend(be, sym, genome_words, ng, packed=packed)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        found = bpos >= 0
        res[name] = {"ms_per_batch": ms, "Mreads_per_s": n / (ms * 1e-3) / 1e6, "extension_jobs": n_jobs,
                     "reads_with_hit": float(found.float().mean().item()),
                     "hit_at_true_position": float(((bpos == torch.clamp(pos - BAND // 2, min=0)) & found).float().mean().item())}
        if name == "reference_layout":
            ref_score, ref_pos = score, bpos
        else:
            res[name]["identical_to_reference_layout"] = bool(torch.equal(score, ref_score) and torch.equal(bpos, ref_pos))
        del idx, be
    # the same batch through nvBowtie's own single-end driver (Aligner::best_approx: seeding passes, randomized hit selection,
    # band-31 quality-aware extension, give-up counters, re-seeding, MAPQ, traceback) -- the reference's policy end to end
    from nvbio_amd import aligner as AL, select as SEL
    names = SEL.pack_names(["r%d" % i for i in range(n)], dev)
    prm = AL.Params(hits_stride=16, batch_size=n)
    for name, idx in (("nvbowtie_best_approx", fmi), ("nvbowtie_best_approx_line_native", "dimer"), ("nvbowtie_best_approx_line_native_ktab8", "dimer8"), ("nvbowtie_best_approx_line_native_trimer", "trimer"),
                      ("nvbowtie_best_approx_line_native_ktab12_ssa1", "dimer12"),
                      ("nvbowtie_best_approx_ktab12_ssa1", 12), ("nvbowtie_best_approx_ktab15_ssa1", 15)):
        if idx == "dimer":                             # the line-native two-symbol index next to the reference layout (11 GB at 3 Gbp)
            idx = fmi.with_dimer()
        elif idx == "dimer8":                          # + the 512 KB prefix table that lives in L2
            idx = fmi.with_dimer().with_ktab(8)
        elif idx == "trimer":                          # + the three-symbol arrays (32 GB at 3 Gbp)
            idx = fmi.with_dimer().with_trimer()
        elif idx == "dimer12":
            idx = fmi.with_dimer().with_ktab(12).with_dense_ssa(1)
        elif not hasattr(idx, "length"):               # HBM-capacity options: 4^k-entry k-mer table (0.13 / 8.6 GB) + the full suffix array (12 GB)
            idx = fmi.with_ktab(idx).with_dense_ssa(1)
        run = lambda st=False: AL.best_approx(idx, None, sym, genome_words, ng, prm, names=names, packed=packed, stage_times=st)
        ms = _timed(run, reps=2)
        r = run(True)
        loc = (r["best"][0] >> 32) & 0xFFFFFFFF
        aligned = loc != 0xFFFFFFFF
        res[name] = {"ms_per_batch": ms, "Mreads_per_s": n / ms / 1e3, "extensions": r["stats"]["extensions"], "dp_jobs": r.get("dp_jobs"), "rounds": r["stats"]["rounds"],
                     "queue_per_seeding_pass": r["stats"]["queue"], "aligned": float(aligned.float().mean().item()),
                     "best_at_true_position": float((aligned & ((loc - pos).abs() <= 2)).float().mean().item()),
                     "mapq_ge_23": float((r["mapq"] >= 23).float().mean().item()), "stage_ms": {k: round(v, 3) for k, v in r["stats"]["ms"].items()}}
        if name == "nvbowtie_best_approx":
            ref_best, ref_mapq, ref_cigar = r["best"], r["mapq"], r["cigar"]
        else:
            res[name]["identical_to_reference_layout"] = bool(torch.equal(r["best"], ref_best) and torch.equal(r["mapq"], ref_mapq) and torch.equal(r["cigar"], ref_cigar))
        del idx, r
    # the same batch through the C++ host driver (include/nvbio_hip/aligner.h: nvbio::bowtie2::cuda::Aligner::best_approx, the
    # north star's "host code stays C++"), entered through tests/cxx/aligner_shim.cpp: no torch between the kernels
    res["cxx_best_approx"] = cxx_driver_leg(a, dev, fmi.with_dimer(), sym, packed, genome_words, ng, names, prm, ref_best, ref_mapq)
    # ... and on the index this GPU's HBM is there for (the default of the config-4 leg below): same driver, same results
    rich, rich_desc = hbm_rich(fmi, dev)
    res["cxx_best_approx_hbm_rich"] = cxx_driver_leg(a, dev, rich, sym, packed, genome_words, ng, names, prm, ref_best, ref_mapq)
    res["cxx_best_approx_hbm_rich"]["index"] = rich_desc
    del rich

    # exact check of a sample against the same glue over the oracle
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_pipeline_gpu import OracleBackend
    m = 20_000
    host = O.FMIndex(parts=(fmi.length, fmi.primary, np.array(fmi.L2, dtype=np.uint32),
                            fmi.bwt_occ.cpu().numpy().view(np.uint32), fmi.ssa.cpu().numpy().view(np.uint32), fmi.sa_int))
    es, ep, _ = P.seed_and_extend(OracleBackend(host, mp, READ_LEN), sym[:m].cpu(), genome_words.cpu(), ng)
    gs, gp, _ = P.seed_and_extend(P.HipBackend(fmi, None, mp, READ_LEN), sym[:m].contiguous(), genome_words, ng)
    ok = bool(torch.equal(gs.cpu(), es) and torch.equal(gp.cpu(), ep))
    if not ok:
        raise SystemExit("parity gate failed: end-to-end driver differs from the oracle")
    res["parity"] = {"checked_reads": m, "bit_exact": ok}
    # ... and of the nvBowtie driver: 2000 reads as their own batch vs the independent numpy driver over the oracle
    import oracle_driver as OD
    m2 = 2000
    prm2 = AL.Params(hits_stride=16, batch_size=m2)
    nm = ["r%d" % i for i in range(m2)]
    rs = AL.best_approx(fmi, None, sym[:m2].contiguous(), genome_words, ng, prm2, names=nm, cigar_stride=64)
    es2 = OD.best_approx(host, None, sym[:m2].cpu().numpy(), genome_words.cpu().numpy().view(np.uint32), ng, prm2, nvb.SmithWatermanScoringScheme(), nm, 2)
    ids = rs["aligned_ids"].cpu().numpy()
    ok2 = bool((rs["best"].cpu().numpy().view(np.uint64) == es2["best"]).all() and (rs["mapq"].cpu().numpy() == es2["mapq"]).all()
               and (rs["cigar"].cpu().numpy()[ids].view(np.uint16) == es2["tb"]["cigar"][: ids.size]).all() and rs["stats"] == es2["stats"])
    if not ok2:
        raise SystemExit("parity gate failed: nvBowtie single-end driver differs from the oracle driver")
    res["parity"]["nvbowtie_driver"] = {"checked_reads": m2, "best_mapq_cigar_stats_equal": ok2}
    # BASELINE config 4 at its full size: 50 M reads = e2e_batches batches of n fresh reads through the C++ single-end driver
    # (nvbio::bowtie2::cuda::Aligner::best_approx; inputs packed in HBM before the timed region), on the HBM-rich index (the default on
    # this GPU) and on the lean line-native index, one batch at a time and with two batches in flight: one host thread, one Aligner and
    # one non-blocking HIP stream per batch in flight, so that one batch's fabric-bound map / locate overlaps the other's VALU-bound
    # select / extend / traceback (what that buys, and why not more: DESIGN.md section 3.7, profiles/r03/cosched_*.txt).
    if a.e2e_batches > 1:
        inputs, truth = [], []
        for b in range(a.e2e_batches):
            symb, posb, _ = P.make_reads(text, n, READ_LEN, seed=0x5EED0040 + b)
            inputs.append(P.pack_read_streams(symb)); truth.append(posb)
            del symb
        tot = n * a.e2e_batches
        c4 = {"reads": tot, "batches": a.e2e_batches, "driver": "nvbio::bowtie2::cuda::Aligner::best_approx (C++, include/nvbio_hip/aligner.h)"}
        ref_results = None
        for flavour in ("reference_layout", "default", "line_native"):
            if flavour == "default":                   # what the loaders build on this device when nothing is said (FMIndexDevice.hbm_default / nvbio::fm_index_hbm)
                idx, desc = hbm_rich(fmi, dev)
            elif flavour == "reference_layout":
                idx, desc = fmi, {"line_native": False, "ktab_k": 0, "sa_int": fmi.sa_int}
            else:
                idx, desc = fmi.with_dimer(), {"line_native": True, "ktab_k": 0, "sa_int": fmi.sa_int}
            serial, sb, sm = cxx_pipelined(dev, idx, inputs, genome_words, ng, names, prm, 1)
            entry = {"index": desc, "serial": serial}
            if sb is not None:
                loc = [(x[0] >> 32) & 0xFFFFFFFF for x in sb]
                entry["aligned"] = sum(int((l != 0xFFFFFFFF).sum().item()) for l in loc) / tot
                entry["best_at_true_position"] = sum(int(((l != 0xFFFFFFFF) & ((l - t).abs() <= 2)).sum().item()) for l, t in zip(loc, truth)) / tot
                co, cb, cm = cxx_pipelined(dev, idx, inputs, genome_words, ng, names, prm, 2)
                if cb is not None:
                    co["identical_to_serial"] = all(torch.equal(x, y) for x, y in zip(cb, sb)) and all(torch.equal(x, y) for x, y in zip(cm, sm))
                entry["two_batches_in_flight"] = co
                del cb, cm
                if flavour == "reference_layout":
                    ref_results = (sb, sm)
                elif ref_results is not None:
                    entry["identical_to_reference_layout"] = all(torch.equal(x, y) for x, y in zip(sb, ref_results[0])) and all(torch.equal(x, y) for x, y in zip(sm, ref_results[1]))
            entry["Mreads_per_s"] = max([v.get("Mreads_per_s", 0.0) for v in (entry.get("serial", {}), entry.get("two_batches_in_flight", {}))])
            c4[flavour] = entry
            del idx, sb, sm
            torch.cuda.empty_cache()
        c4["Mreads_per_s"] = c4["default"]["Mreads_per_s"]              # the figure of the index a user gets by default
        del ref_results
        res["config4_full_size"] = c4
        del inputs, truth
    # BASELINE config 5's shape in the default run: nvBowtie's paired-end driver (2 x 150 bp FR pairs, --local: 20-bp seeds, LOCAL band 31
    # in the quality-aware local scheme, opposite mates by full-matrix DP, paired reduction, MAPQ, tracebacks) on this 3 Gbp index,
    # line-native.  (Its parity sample against the oracle driver is in the extras leg, on a 1 Gbp index with a reverse index too.)
    if a.pairs > 0:
        npairs = a.pairs
        s1, s2, ppos, pflen = P.make_read_pairs(text, npairs, 150, seed=0x5EED0009)
        pnames = SEL.pack_names(["p%d" % i for i in range(npairs)], dev)
        idx = fmi.with_dimer()
        prm5 = AL.Params(hits_stride=32, batch_size=npairs, local=True, seed_len=20, seed_freq=(2, 1.0, 0.75))
        runp = lambda st=False: AL.best_approx_paired(idx, None, s1, s2, genome_words, ng, prm5, names=pnames, stage_times=st)
        msp = _timed(runp, reps=2)
        r = runp(True)
        b0 = r["best"][0]
        conc = (((b0 >> 30) & 1) != 0) & (((b0 >> 31) & 1) == 0)
        a_pos = (b0 >> 32) & 0xFFFFFFFF
        ok_pos = (((a_pos - ppos).abs() <= 3) | ((a_pos - (ppos + pflen - 150)).abs() <= 3)) & conc
        res["config5_shape_paired_end"] = {"pairs": npairs, "index": "line_native", "ms_per_batch": msp, "Mpairs_per_s": npairs / msp / 1e3,
                                           "anchor_extensions": r["stats"]["extensions"], "opposite_dp_jobs": r.get("opposite_dp_jobs"),
                                           "concordant": float(conc.float().mean().item()), "concordant_at_fragment_end": float(ok_pos.float().mean().item()),
                                           "stage_ms": {k: round(v, 3) for k, v in r["stats"]["ms"].items()}}
        res["config5_shape_paired_end"]["cxx"] = cxx_paired_leg(dev, idx, s1, s2, genome_words, ng, pnames, prm5, b0)
        del idx, r, s1, s2
        # BASELINE config 5 at one GPU's share: 200 M pairs over 8 GPUs = 25 M pairs per GPU, through the C++ paired-end driver in batches
        if a.share_pairs > 0:
            res["config5_per_gpu_share"] = config5_share_leg(a, dev, fmi, text, genome_words, ng, pnames, prm5, npairs)
    res["reads"] = n
    res["genome_symbols"] = ng
    return res


def config5_share_leg(a, dev, fmi, text, genome_words, ng, names, prm, batch_pairs):
    """BASELINE config 5 at the share one of 8 GPUs gets (25 M of 200 M pairs, 2 x 150 bp, LOCAL band 31): the C++ paired-end driver over
    share_pairs / batch_pairs batches of fresh pairs (inputs resident in HBM), one batch at a time and two in flight; the 32-byte pair
    records (io::BestPairedAlignments) of every batch are produced on the device.  Host <-> device transfers of one batch (BASELINE.md
    section 3: reported separately, never inside `value`): packed reads + qualities in, pair records out, through pinned host memory."""
    import ctypes as C
    from nvbio_amd import pipeline as P
    shim = C.CDLL(os.path.join(ROOT, "tests", "cxx", "libaligner_shim.so"))
    n, L = batch_pairs, 150
    nb = max(1, a.share_pairs // n)
    idx, desc = hbm_rich(fmi, dev)

    class PairBatch(C.Structure):
        _fields_ = [("rev_words", C.c_void_p * 2), ("rev_begin", C.c_void_p * 2), ("fwrc_words", C.c_void_p * 2), ("both_words", C.c_void_p)]

    class ShimPeParams(C.Structure):
        _fields_ = [("pe_policy", C.c_int32)] + [(k, C.c_uint32) for k in ("pe_overlap", "pe_unpaired", "pe_discordant", "min_frag_len", "max_frag_len")]
    keep, arr = [], (PairBatch * nb)()
    conc_at_true = 0
    truth = []
    for b in range(nb):
        s1, s2, ppos, pflen = P.make_read_pairs(text, n, L, seed=0x5EED0100 + b)
        pk = [P.pack_read_streams(x) for x in (s1, s2)]
        both = torch.cat([pk[0][1], pk[1][1]])
        keep.append((pk, both)); truth.append((ppos, pflen))
        for m in range(2):
            arr[b].rev_words[m] = pk[m][0].words.data_ptr(); arr[b].rev_begin[m] = pk[m][0].begin.data_ptr(); arr[b].fwrc_words[m] = pk[m][1].data_ptr()
        arr[b].both_words = both.data_ptr()
        del s1, s2
    pk0 = keep[0][0]
    mate_offset = pk0[0][1].numel() * 8
    quals = torch.full((2 * n * L + 8,), 30, dtype=torch.uint8, device=dev)
    both_q = torch.full((mate_offset + 2 * n * L + 8,), 30, dtype=torch.uint8, device=dev)
    arena, nidx = names
    scheme = nvb.SmithWatermanScoringScheme.local() if prm.local else nvb.SmithWatermanScoringScheme()
    sp = _shim_params(prm, scheme)
    pp = ShimPeParams(prm.pe_policy, int(prm.pe_overlap), int(prm.pe_unpaired), int(prm.pe_discordant), prm.min_frag_len, prm.max_frag_len)
    u64x2 = lambda v: (C.c_uint64 * 2)(*v)
    vp = lambda t: C.c_void_p(t.data_ptr())
    records = [torch.zeros((4, n), dtype=torch.int64, device=dev) for _ in range(nb)]
    rec_ptrs = (C.c_void_p * nb)(*[t.data_ptr() for t in records])
    fs = idx.struct()
    out = {"pairs": n * nb, "batches": nb, "pairs_per_batch": n, "read_len": L, "index": desc,
           "driver": "nvbio::bowtie2::cuda::Aligner::best_approx(PairedReadBatch) (C++, include/nvbio_hip/aligner.h)", "pair_record_bytes": 32}
    ref = None
    for key, workers in (("serial", 1), ("two_batches_in_flight", 2)):
        ms, stats = (C.c_double * 1)(), (C.c_uint64 * 2)()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()               # the C++ drivers allocate their own workspaces: hand them what torch's allocator has cached
        rc = shim.nvbio_aligner_best_approx_paired_pipelined(
            C.byref(fs), None, C.c_uint32(n), C.c_uint32(L), C.c_uint32(nb), arr,
            u64x2([pk0[0][0].words.numel(), pk0[1][0].words.numel()]), u64x2([pk0[0][1].numel(), pk0[1][1].numel()]),
            vp(quals), C.c_uint64(quals.numel()), vp(arena), vp(nidx), C.c_uint64(keep[0][1].numel()), C.c_uint64(mate_offset), vp(both_q), C.c_uint64(both_q.numel()),
            vp(genome_words), C.c_uint64(genome_words.numel()), C.c_uint32(ng), C.byref(sp), C.byref(pp),
            C.c_uint32(workers), ms, rec_ptrs, stats)
        torch.cuda.synchronize()
        if rc != 0:
            out[key] = {"error": "nvbio_aligner_best_approx_paired_pipelined returned %d" % rc}
            continue
        out[key] = {"host_threads": workers, "ms_total": ms[0], "Mpairs_per_s": n * nb / ms[0] / 1e3,
                    "ms_per_batch": ms[0] / nb, "anchor_extensions": int(stats[0])}
        if ref is None:
            ref = [t.clone() for t in records]
            conc = tru = 0
            for t, (ppos, pflen) in zip(records, truth):
                b0 = t[0]
                c = (((b0 >> 30) & 1) != 0) & (((b0 >> 31) & 1) == 0)
                apos = (b0 >> 32) & 0xFFFFFFFF
                conc += int(c.sum().item())
                tru += int(((((apos - ppos).abs() <= 3) | ((apos - (ppos + pflen - L)).abs() <= 3)) & c).sum().item())
            out["concordant"] = conc / (n * nb); out["concordant_at_fragment_end"] = tru / (n * nb)
        else:
            out[key]["identical_to_serial"] = all(torch.equal(x, y) for x, y in zip(records, ref))
    # host <-> device traffic of one batch, through pinned memory: 4-bit reads (reversed stream) + a quality byte per base in, 32-byte records out
    rd = [pk0[m][0].words for m in range(2)]
    h_reads = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in rd]
    h_quals = torch.empty(2 * n * L, dtype=torch.uint8).pin_memory()
    h_rec = torch.empty((4, n), dtype=torch.int64).pin_memory()
    d_reads = [torch.empty_like(t) for t in rd]
    d_quals = torch.empty(2 * n * L, dtype=torch.uint8, device=dev)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for rep in range(2):                                   # the first pass maps the pinned pages
        e[0].record()
        for hsrc, d in zip(h_reads, d_reads):
            d.copy_(hsrc, non_blocking=True)
        d_quals.copy_(h_quals, non_blocking=True)
        e[1].record()
        e[2].record()
        h_rec.copy_(records[0], non_blocking=True)
        e[3].record()
        torch.cuda.synchronize()
    h2d_b = sum(t.numel() * 4 for t in rd) + 2 * n * L
    d2h_b = 32 * n
    h2d_ms, d2h_ms = e[0].elapsed_time(e[1]), e[2].elapsed_time(e[3])
    # the derived streams the stages read (forward + reverse-complement copies, both mates in one stream) are built on the device
    t0 = time.perf_counter()
    s1, s2, _, _ = P.make_read_pairs(text, n, L, seed=0x5EED0100)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    pk = [P.pack_read_streams(x) for x in (s1, s2)]; torch.cat([pk[0][1], pk[1][1]])
    torch.cuda.synchronize(); t2 = time.perf_counter()
    best = out.get("two_batches_in_flight", out.get("serial", {}))
    comp_ms = best.get("ms_per_batch")
    out["host_transfers_per_batch"] = {"h2d_bytes": h2d_b, "h2d_ms": h2d_ms, "h2d_GBs": h2d_b / h2d_ms / 1e6, "d2h_bytes": d2h_b, "d2h_ms": d2h_ms, "d2h_GBs": d2h_b / d2h_ms / 1e6,
                                       "device_side_repacking_ms": (t2 - t1) * 1e3,
                                       "note": "pinned host memory, one stream; h2d = both mates' packed reads + a quality byte per base, d2h = the 32-byte pair records"}
    if comp_ms:
        out["host_transfers_per_batch"]["Mpairs_per_s_if_transfers_were_serialised_with_compute"] = n / (comp_ms + h2d_ms + d2h_ms) / 1e3
        out["host_transfers_per_batch"]["Mpairs_per_s_if_transfers_overlap_compute"] = n / max(comp_ms, h2d_ms + d2h_ms) / 1e3
    return out


def _shim_params(p, scheme):
    """tests/cxx/aligner_shim.cpp's shim_params (nvBowtie's Params as the shim takes them) for an nvbio_amd.aligner.Params."""
    import ctypes as C

    class ShimParams(C.Structure):
        _fields_ = [(k, C.c_uint32) for k in ("local", "randomized", "top_seed", "max_effort_init", "max_effort", "min_ext", "max_ext", "max_reseed", "rep_seeds",
                                              "max_hits", "allow_sub", "subseed_len", "seed_len", "seed_freq_type", "min_read_len", "max_dist", "no_multi_hits",
                                              "batch_size", "hits_stride")] + \
                   [("seed_freq_k", C.c_float), ("seed_freq_m", C.c_float), ("match", C.c_int32), ("score_min_type", C.c_int32),
                    ("score_min_k", C.c_float), ("score_min_m", C.c_float), ("finish", C.c_uint32), ("edit_distance", C.c_uint32)]
    return ShimParams(int(p.local), int(p.randomized), p.top_seed, p.max_effort_init, p.max_effort, p.min_ext, p.max_ext, p.max_reseed, p.rep_seeds, p.max_hits,
                      p.allow_sub, p.subseed_len, p.seed_len, p.seed_freq[0], p.min_read_len, p.max_dist, int(p.no_multi_hits), p.batch_size, p.hits_stride or 0,
                      p.seed_freq[1], p.seed_freq[2], scheme.m_match, scheme.m_score_min[0], scheme.m_score_min[1], scheme.m_score_min[2], 0, 1 if getattr(p, "scoring_mode", "sw") == "ed" else 0)


def cxx_paired_leg(dev, idx, s1, s2, genome_words, ng, names, prm, ref_best0):
    """The C++ paired-end driver (Aligner::best_approx over a PairedReadBatch, include/nvbio_hip/aligner.h) on the same pairs: mean wall
    time of 3 batches with one Aligner object (tests/cxx/aligner_shim.cpp: nvbio_aligner_best_approx_paired_timed)."""
    import ctypes as C
    from nvbio_amd import pipeline as P
    shim_path = os.path.join(ROOT, "tests", "cxx", "libaligner_shim.so")
    if not os.path.exists(shim_path):
        return {"error": "tests/cxx/libaligner_shim.so is missing (python __graft_entry__.py builds it)"}
    shim = C.CDLL(shim_path)
    n, L = s1.shape
    packed = [P.pack_read_streams(s) for s in (s1, s2)]
    quals = torch.full((2 * n * L + 8,), 30, dtype=torch.uint8, device=dev)
    both = torch.cat([packed[0][1], packed[1][1]]); mate_offset = packed[0][1].numel() * 8
    both_q = torch.full((mate_offset + 2 * n * L + 8,), 30, dtype=torch.uint8, device=dev)
    arena, nidx = names
    scheme = nvb.SmithWatermanScoringScheme.local() if prm.local else nvb.SmithWatermanScoringScheme()

    class ShimPeParams(C.Structure):
        _fields_ = [("pe_policy", C.c_int32)] + [(k, C.c_uint32) for k in ("pe_overlap", "pe_unpaired", "pe_discordant", "min_frag_len", "max_frag_len")]
    p = prm
    sp = _shim_params(prm, scheme)
    pp = ShimPeParams(p.pe_policy, int(p.pe_overlap), int(p.pe_unpaired), int(p.pe_discordant), p.min_frag_len, p.max_frag_len)
    pair_ptrs = lambda ts: (C.c_void_p * 2)(*[t.data_ptr() for t in ts])
    u64x2 = lambda v: (C.c_uint64 * 2)(*v)
    vp = lambda t: C.c_void_p(t.data_ptr())
    fs = idx.struct()
    ms, stage, stats = (C.c_double * 1)(), (C.c_double * 10)(), (C.c_uint64 * 12)()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()                   # the C++ driver allocates its own workspace: give it what torch's allocator has cached
    rc = shim.nvbio_aligner_best_approx_paired_timed(
        C.byref(fs), None, C.c_uint32(n), C.c_uint32(L),
        pair_ptrs([packed[0][0].words, packed[1][0].words]), u64x2([packed[0][0].words.numel(), packed[1][0].words.numel()]), pair_ptrs([packed[0][0].begin, packed[1][0].begin]),
        pair_ptrs([packed[0][1], packed[1][1]]), u64x2([packed[0][1].numel(), packed[1][1].numel()]), vp(quals), C.c_uint64(quals.numel()), vp(arena), vp(nidx),
        vp(both), C.c_uint64(both.numel()), C.c_uint64(mate_offset), vp(both_q), C.c_uint64(both_q.numel()),
        vp(genome_words), C.c_uint64(genome_words.numel()), C.c_uint32(ng), C.byref(sp), C.byref(pp), C.c_uint32(3), ms, stage, stats)
    if rc != 0:
        return {"error": "nvbio_aligner_best_approx_paired_timed returned %d" % rc}
    return {"driver": "nvbio::bowtie2::cuda::Aligner::best_approx(PairedReadBatch) (include/nvbio_hip/aligner.h)", "ms_per_batch": ms[0], "Mpairs_per_s": n / ms[0] / 1e3,
            "anchor_extensions": int(stats[0]), "rounds": int(stats[1]),
            "stage_ms": {k: round(stage[i], 3) for i, k in enumerate(("map", "select_init", "select", "locate", "anchor_score", "opposite_score", "reduce", "mapq", "traceback", "finish"))}}


def cxx_driver_leg(a, dev, idx, sym, packed, genome_words, ng, names, prm, ref_best, ref_mapq):
    """nvbio::bowtie2::cuda::Aligner::best_approx (C++ over the C-ABI) on the e2e batch: mean wall time per batch of `reps` batches
    with one Aligner object, per-stage device times from one more batch, and its results compared with the Python driver's."""
    import ctypes as C
    shim_path = os.path.join(ROOT, "tests", "cxx", "libaligner_shim.so")
    if not os.path.exists(shim_path):
        return {"error": "tests/cxx/libaligner_shim.so is missing (python __graft_entry__.py builds it)"}
    shim = C.CDLL(shim_path)
    n, L = sym.shape
    reads_rev, fwrc = packed
    quals = torch.full((2 * n * L + 8,), 30, dtype=torch.uint8, device=dev)
    arena, nidx = names
    scheme = nvb.SmithWatermanScoringScheme()

    sp = _shim_params(prm, scheme)
    fs = idx.struct()
    vp = lambda t: C.c_void_p(t.data_ptr())
    best = torch.zeros((2, n), dtype=torch.int64, device=dev)
    mapq = torch.zeros(n, dtype=torch.uint8, device=dev)
    ms, stage, stats = (C.c_double * 1)(), (C.c_double * 9)(), (C.c_uint64 * 4)()
    torch.cuda.synchronize()
    rc = shim.nvbio_aligner_best_approx_timed(C.byref(fs), None, C.c_uint32(n), C.c_uint32(L), vp(reads_rev.words), C.c_uint64(reads_rev.words.numel()), vp(reads_rev.begin),
                                              vp(fwrc), C.c_uint64(fwrc.numel()), vp(quals), C.c_uint64(quals.numel()), vp(arena), vp(nidx),
                                              vp(genome_words), C.c_uint64(genome_words.numel()), C.c_uint32(ng), C.byref(sp), C.c_uint32(3), ms, stage, vp(best), vp(mapq), stats)
    if rc != 0:
        return {"error": "nvbio_aligner_best_approx_timed returned %d" % rc}
    names9 = ("map", "select_init", "select", "locate", "score", "reduce", "mapq", "traceback", "finish")
    return {"driver": "nvbio::bowtie2::cuda::Aligner::best_approx (include/nvbio_hip/aligner.h)", "ms_per_batch": ms[0], "Mreads_per_s": n / ms[0] / 1e3,
            "extensions": int(stats[0]), "rounds": int(stats[1]), "dp_jobs": int(stats[3]),
            "stage_ms": {k: round(stage[i], 3) for i, k in enumerate(names9)},
            "identical_to_python_driver": bool(torch.equal(best, ref_best) and torch.equal(mapq, ref_mapq))}


def cxx_pipelined(dev, idx, batches, genome_words, ng, names, prm, workers, reps=2):
    """`len(batches)` batches of reads through the C++ single-end driver with `workers` host threads / HIP streams sharing the device
    (tests/cxx/aligner_shim.cpp: nvbio_aligner_best_approx_pipelined).
    batches: [pack_read_streams(sym), ...].  Returns (dict, bests, mapqs)."""
    import ctypes as C
    shim = C.CDLL(os.path.join(ROOT, "tests", "cxx", "libaligner_shim.so"))
    nb = len(batches)
    n = int(batches[0][0].begin.numel()); L = READ_LEN
    quals = torch.full((2 * n * L + 8,), 30, dtype=torch.uint8, device=dev)
    arena, nidx = names
    sp = _shim_params(prm, nvb.SmithWatermanScoringScheme())
    fs = idx.struct()
    vp = lambda t: C.c_void_p(t.data_ptr())
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    best = [torch.zeros((2, n), dtype=torch.int64, device=dev) for _ in range(nb)]
    mapq = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(nb)]
    ms = (C.c_double * 1)()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    rc = shim.nvbio_aligner_best_approx_pipelined(
        C.byref(fs), None, C.c_uint32(n), C.c_uint32(L), C.c_uint32(nb),
        ptrs([b[0].words for b in batches]), C.c_uint64(batches[0][0].words.numel()), ptrs([b[0].begin for b in batches]),
        ptrs([b[1] for b in batches]), C.c_uint64(batches[0][1].numel()), vp(quals), C.c_uint64(quals.numel()), vp(arena), vp(nidx),
        vp(genome_words), C.c_uint64(genome_words.numel()), C.c_uint32(ng), C.byref(sp),
        C.c_uint32(workers), C.c_uint32(reps), ms, ptrs(best), ptrs(mapq))
    torch.cuda.synchronize()
    if rc != 0:
        return {"error": "nvbio_aligner_best_approx_pipelined returned %d" % rc}, None, None
    return {"host_threads": workers, "ms_total": ms[0], "Mreads_per_s": n * nb / ms[0] / 1e3}, best, mapq


def hbm_rich(fmi, dev):
    """The index the loaders build on this device when nothing is said -- the library's own policy (nvbio_amd.fmindex.FMIndexDevice.hbm_default =
    nvbio::fm_index_hbm::build of the C++ host layer): line-native two-symbol records, the densest suffix array and the largest k-mer table that fit
    35 % of the free memory (3 Gbp on a 288 GB MI355X: the whole suffix array, 12 GB, and every 16-mer's range, 34 GB).  Results stay bit-identical
    (checked by the callers)."""
    torch.cuda.empty_cache()                   # (what torch's allocator has cached counts as free)
    idx, desc = fmi.hbm_default()
    desc = dict(desc, ktab_bytes=(4 ** desc["ktab_k"]) * 8 if desc["ktab_k"] else 0, ssa_bytes=int(idx.ssa.numel()) * 4 if idx.ssa is not None else 0,
                dimer_bytes=int(idx.dimer.numel()) * 4 if idx.dimer is not None else 0)
    return idx, desc


def rank_leg(a, dev, fmi):
    """rank(i,c) point queries at uniform random i: algorithmic 40 B per query."""
    ng = fmi.length
    bwt_occ = fmi.bwt_occ
    q = a.rank_queries
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED0003)
    k = torch.randint(0, ng, (q,), dtype=torch.int64, generator=g, device=dev).to(torch.int32)
    c = torch.randint(0, 4, (q,), dtype=torch.uint8, generator=g, device=dev)
    r = nvb.rank(fmi, k, c)          # warm-up + property check: rank <= k+1, and sums over c
    torch.cuda.synchronize()
    kk = (k.to(torch.int64) & 0xFFFFFFFF)
    assert bool(((r.to(torch.int64) & 0xFFFFFFFF) <= kk + 1).all())
    reps = 5
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in evs:
        e0.record()
        nvb.rank(fmi, k, c)
        e1.record()
    torch.cuda.synchronize()
    ms = sum(e0.elapsed_time(e1) for e0, e1 in evs) / reps
    gbs = q * RANK_BYTES_PER_QUERY / (ms * 1e-3) / 1e9
    traffic = measured_traffic("fm_rank_kernel")
    res = {"kernel": "fm_rank_kernel", "bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "frac": gbs / HBM_PEAK_GBS, "traffic": traffic, "traffic_round": counters_round("fm_rank_kernel"), "kernel_ms": ms, "queries": q, "index_symbols": ng,
           "index_bytes": int(bwt_occ.numel()) * 4, "Mqueries_per_s": q / (ms * 1e-3) / 1e6}
    if traffic:
        # what the memory system actually moved (PMC, profiles/traffic.json, measured at the default query count): every query
        # misses to a 128-byte fabric request although it needs 32 bytes of it
        scale = q / 268435456.0
        res["traffic_GBs"] = traffic * scale / (ms * 1e-3) / 1e9
        res["traffic_frac_of_hbm_peak"] = res["traffic_GBs"] / HBM_PEAK_GBS
    res["random_lines_per_s_G"] = q / (ms * 1e-3) / 1e9
    res["random_line_limit_G"] = 53.0          # tools/gather_probe.hip (profiles/r01/gather_probe.txt): the chip's random 128-B line rate
    # how to read `frac`: a point query needs 32 bytes of the 128-byte line the fabric moves for it, and the kernel issues those lines at
    # request_rate_frac of the rate the chip sustains for random lines -- frac = useful_fraction_of_line x (moved bytes / HBM peak)
    res["useful_fraction_of_line"] = 32.0 / 128.0
    res["request_rate_frac"] = res["random_lines_per_s_G"] / res["random_line_limit_G"]
    res["order"] = "shuffled"
    res["note"] = ("uniform random point queries, shuffled: one 128-B fabric request per query is the floor (~53 G/s on this chip), so 40 "
                   "algorithmic bytes per query cannot exceed ~0.27 of HBM peak in this order; `sorted_order` is the same query set sorted by row, the "
                   "other order the reference's own test runs (fmindex_test.cu:666-716), where neighbouring queries share lines")
    # the same queries sorted by row (same kernel, same results up to the permutation)
    ks, perm = torch.sort(k.to(torch.int64) & 0xFFFFFFFF)
    ks, cs = ks.to(torch.int32), c[perm].contiguous()
    rs = nvb.rank(fmi, ks, cs)
    torch.cuda.synchronize()
    assert bool(torch.equal(rs, r[perm]))
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in evs:
        e0.record()
        nvb.rank(fmi, ks, cs)
        e1.record()
    torch.cuda.synchronize()
    ms_s = sum(e0.elapsed_time(e1) for e0, e1 in evs) / reps
    gbs_s = q * RANK_BYTES_PER_QUERY / (ms_s * 1e-3) / 1e9
    sorted_traffic = measured_traffic("fm_rank_kernel_sorted")
    res["sorted_order"] = {"kernel_ms": ms_s, "algorithmic_GBs": gbs_s, "Mqueries_per_s": q / (ms_s * 1e-3) / 1e6, "identical_to_shuffled": True,
                           "traffic": sorted_traffic, "traffic_round": counters_round("fm_rank_kernel_sorted"),
                           "note": "NOT a roofline figure: ~11 consecutive queries share a 128-B line and L2 serves the repeats, so algorithmic bytes (40 per query) over "
                                   "time can pass the HBM peak; `traffic` is what the fabric moved for this order (TCC_EA0_RDREQ pass, profiles/traffic.json), "
                                   "null until that pass has been taken"}
    if sorted_traffic:
        res["sorted_order"]["traffic_GBs"] = sorted_traffic * (q / 268435456.0) / (ms_s * 1e-3) / 1e9
        res["sorted_order"]["traffic_frac_of_hbm_peak"] = res["sorted_order"]["traffic_GBs"] / HBM_PEAK_GBS
    # the same shuffled point queries on the line-native index (plane records: the row's 128-byte line holds its nibble and its counters)
    try:
        fd = fmi.with_dimer()
        rd = nvb.rank(fd, k, c)
        torch.cuda.synchronize()
        same = bool(torch.equal(rd, r))
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in evs:
            e0.record()
            nvb.rank(fd, k, c)
            e1.record()
        torch.cuda.synchronize()
        ms_d = sum(e0.elapsed_time(e1) for e0, e1 in evs) / reps
        res["line_native"] = {"kernel_ms": ms_d, "achieved": q * RANK_BYTES_PER_QUERY / (ms_d * 1e-3) / 1e9, "frac": q * RANK_BYTES_PER_QUERY / (ms_d * 1e-3) / 1e9 / HBM_PEAK_GBS,
                              "Mqueries_per_s": q / (ms_d * 1e-3) / 1e6, "random_lines_per_s_G": q / (ms_d * 1e-3) / 1e9, "identical_to_reference_layout": same,
                              "note": "a point query is one 128-byte line on either layout; the line-native index pays off where a step needs both ends of a range or two symbols"}
        del fd, rd
    except Exception as e:     # noqa: BLE001 -- reported, the leg continues
        res["line_native"] = {"error": "%s: %s" % (type(e).__name__, e)}
    return res


def seed_leg(a, dev, fmi, text, build_s):
    """Backward search (match) of 22-bp seeds and locate of their first SA row (SURVEY.md 8d config
    3-ii).  A sample is checked bit-exactly against the oracle run on a host copy of the same
    index; the oracle also counts the algorithmic index bytes per seed."""
    import numpy as np
    from oracle import pyoracle as O
    ng = fmi.length
    seeds = W.make_seeds(text, a.seeds, 22)
    ranges = nvb.match(fmi, seeds)
    torch.cuda.synchronize()
    reps = 5
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in evs:
        e0.record(); nvb.match(fmi, seeds, out=ranges); e1.record()
    torch.cuda.synchronize()
    match_ms = sum(e0.elapsed_time(e1) for e0, e1 in evs) / reps
    # locate the first row of every non-empty range
    ok = (ranges[:, 0].to(torch.int64) & 0xFFFFFFFF) <= (ranges[:, 1].to(torch.int64) & 0xFFFFFFFF)
    rows = ranges[:, 0][ok].contiguous()
    pos = nvb.locate(fmi, rows)
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in evs:
        e0.record(); nvb.locate(fmi, rows, out=pos); e1.record()
    torch.cuda.synchronize()
    locate_ms = sum(e0.elapsed_time(e1) for e0, e1 in evs) / reps
    # parity + algorithmic bytes on a sample, by the oracle on a host copy of the same index
    m = min(a.seeds, 1_000_000)
    host = O.FMIndex(parts=(fmi.length, fmi.primary, np.array(fmi.L2, dtype=np.uint32),
                            fmi.bwt_occ.cpu().numpy().view(np.uint32), fmi.ssa.cpu().numpy().view(np.uint32), fmi.sa_int))
    sub = nvb.PackedStringSet(seeds.words, seeds.bits, seeds.big_endian, seeds.begin[:m].contiguous(), None, 22)
    er, nbytes = host.match(O.StringSet.from_device(sub), want_bytes=True)
    exact = bool((ranges[:m].cpu().numpy().view(np.uint32) == er).all())
    mr = min(int(rows.numel()), 1_000_000)
    ep, steps = host.locate(rows[:mr].cpu().numpy().view(np.uint32), want_steps=True)
    exact = exact and bool((pos[:mr].cpu().numpy().view(np.uint32) == ep).all())
    if not exact:
        raise SystemExit("parity gate failed: FM-index match/locate differ from the oracle")
    # MI355X-native options that spend HBM capacity to remove dependent gathers; ranges and
    # positions are bit-identical (checked below): a 12-mer table for match (128 MiB) and denser
    # suffix-array samples for locate (sa_int 4: 3 GB, sa_int 1 = the full SA: 12 GB at 3 Gbp)
    def timed(fn):
        fn(); torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in ev) / reps
    options = {}
    # the line-native two-symbol index (nvbio_amd/csrc/fmindex_dimer.h): two symbols per backward-search step and two text
    # positions per locate step; ranges and positions must be bit-identical
    t0 = time.perf_counter()
    fdim = fmi.with_dimer()
    torch.cuda.synchronize()
    dimer_s = time.perf_counter() - t0
    r2 = torch.empty_like(ranges)
    p2 = torch.empty_like(pos)
    dm_ms = timed(lambda: nvb.match(fdim, seeds, out=r2))
    dl_ms = timed(lambda: nvb.locate(fdim, rows, out=p2))
    srt = torch.sort(rows.to(torch.int64) & 0xFFFFFFFF).values.to(torch.int32)
    ps = torch.empty_like(pos)
    line_native = {"index_bytes": int(fdim.dimer.numel()) * 4, "build_s": dimer_s,
                   "match": {"kernel": "fm_match_kernel", "kernel_ms": dm_ms, "Mseeds_per_s": a.seeds / (dm_ms * 1e-3) / 1e6,
                             "identical": bool(torch.equal(r2, ranges))},
                   "locate": {"kernel": "fm_locate_kernel", "kernel_ms": dl_ms, "Mrows_per_s": rows.numel() / (dl_ms * 1e-3) / 1e6,
                              "identical": bool(torch.equal(p2, pos)),
                              "sorted_rows_kernel_ms": timed(lambda: nvb.locate(fdim, srt, out=ps))}}
    # what the reference's SA-row sort before locate (aligner_best_approx.h:735-741: sort_hi_bits) would cost here, to set against
    # the gain of sorted rows above: the drivers do not sort, because the gain is smaller than the sort
    from nvbio_amd import select as SEL
    line_native["locate"]["sort_hi_bits_ms"] = timed(lambda: SEL.sort_hi_bits(rows))
    fdk = fdim.with_ktab(12)
    dk_ms = timed(lambda: nvb.match(fdk, seeds, out=r2))
    line_native["match_ktab12"] = {"kernel_ms": dk_ms, "Mseeds_per_s": a.seeds / (dk_ms * 1e-3) / 1e6, "identical": bool(torch.equal(r2, ranges))}
    del fdk
    # the largest table (every 16-mer, 34 GB): a 22-bp seed is one look-up + three two-symbol steps.  A seed is then ~4 fabric requests, so the
    # figure that says how close the kernel is to the chip is requests/s against the measured random-request rate (~53 G/s), not bytes against HBM
    torch.cuda.empty_cache()
    if torch.cuda.mem_get_info(dev)[0] > (48 << 30) and ng > (1 << 28):
        fdk = fdim.with_ktab(16)
        dk_ms = timed(lambda: nvb.match(fdk, seeds, out=r2))
        rate = a.seeds / (dk_ms * 1e-3)
        line_native["match_ktab16"] = {"kernel_ms": dk_ms, "Mseeds_per_s": rate / 1e6, "table_bytes": int(fdk.ktab.numel()) * 4, "identical": bool(torch.equal(r2, ranges)),
                                       "fabric_requests_per_seed_model": 4, "G_requests_per_s": 4 * rate / 1e9, "frac_of_random_request_rate": 4 * rate / 53e9}
        del fdk
    # a 4^8-entry table is 512 KB: resident in every XCD's L2, it replaces the four widest pair steps (8 line requests) of a seed
    fd8 = fdim.with_ktab(8)
    d8_ms = timed(lambda: nvb.match(fd8, seeds, out=r2))
    line_native["match_ktab8_l2_resident"] = {"kernel_ms": d8_ms, "Mseeds_per_s": a.seeds / (d8_ms * 1e-3) / 1e6, "table_bytes": int(fd8.ktab.numel()) * 4,
                                              "identical": bool(torch.equal(r2, ranges))}
    del fd8
    # three symbols per step on the 64 per-trimer rank arrays (32 GB at 3 Gbp: an HBM-capacity option)
    t0 = time.perf_counter()
    ftri = fdim.with_trimer()
    torch.cuda.synchronize()
    tri_s = time.perf_counter() - t0
    t3_ms = timed(lambda: nvb.match(ftri, seeds, out=r2))
    line_native["match_trimer"] = {"kernel_ms": t3_ms, "Mseeds_per_s": a.seeds / (t3_ms * 1e-3) / 1e6, "index_bytes": int(ftri.trimer.numel()) * 4, "build_s": tri_s,
                                   "identical": bool(torch.equal(r2, ranges))}
    del ftri
    ref_sorted_ms = timed(lambda: nvb.locate(fmi, srt, out=ps))
    del fdim, r2, p2, ps, srt
    if not all(v["identical"] for v in line_native.values() if isinstance(v, dict)):
        raise SystemExit("parity gate failed: the line-native index changes match/locate results")
    fk = fmi.with_ktab(12)
    r2 = torch.empty_like(ranges)
    options["match_ktab12"] = {"kernel_ms": timed(lambda: nvb.match(fk, seeds, out=r2)), "table_bytes": int(fk.ktab.numel()) * 4}
    options["match_ktab12"]["Mseeds_per_s"] = a.seeds / (options["match_ktab12"]["kernel_ms"] * 1e-3) / 1e6
    options["match_ktab12"]["identical"] = bool(torch.equal(r2, ranges))
    del fk, r2
    for K in (4, 1):
        t0 = time.perf_counter()
        fd = fmi.with_dense_ssa(K)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        p2 = torch.empty_like(pos)
        ms = timed(lambda: nvb.locate(fd, rows, out=p2))
        options["locate_sa_int%d" % K] = {"kernel_ms": ms, "Mrows_per_s": rows.numel() / (ms * 1e-3) / 1e6, "ssa_bytes": int(fd.ssa.numel()) * 4,
                                          "densify_s": dt, "identical": bool(torch.equal(p2, pos))}
        del fd, p2
    if not all(o["identical"] for o in options.values()):
        raise SystemExit("parity gate failed: accelerated match/locate differ from the plain kernels")
    bytes_per_seed = nbytes / m + 6 + 8
    bytes_per_loc = 32.0 * steps / mr + 4 + 8
    mgbs = a.seeds * bytes_per_seed / (match_ms * 1e-3) / 1e9
    lgbs = rows.numel() * bytes_per_loc / (locate_ms * 1e-3) / 1e9
    # counter traffic of the line-native kernels: fabric requests per unit from the committed PMC pass x this launch's units
    rq = measured_counter("fm_match_kernel<line_native>", "rdreq_128B_per_seed")
    if rq is not None:
        line_native["match"]["traffic"] = int(a.seeds * (rq * 128 + 8))
        line_native["match"]["traffic_over_algorithmic"] = (rq * 128 + 8) / bytes_per_seed
        line_native["match"]["traffic_round"] = counters_round("fm_match_kernel<line_native>")
    rq = measured_counter("fm_locate_kernel<line_native>", "rdreq_128B_per_row")
    if rq is not None:
        line_native["locate"]["traffic"] = int(rows.numel() * (rq * 128 + 4))
        line_native["locate"]["traffic_over_algorithmic"] = (rq * 128 + 4) / bytes_per_loc
        line_native["locate"]["traffic_round"] = counters_round("fm_locate_kernel<line_native>")
    # the line-native figures priced in the SAME algorithmic bytes (what the reference's walk would touch): the index does the
    # job in fewer, fuller lines, so the fraction says how close the seeding stage is to what 8 TB/s could do for that walk
    for leg, nunits, bpu in (("match", a.seeds, bytes_per_seed), ("locate", rows.numel(), bytes_per_loc)):
        g = nunits * bpu / (line_native[leg]["kernel_ms"] * 1e-3) / 1e9
        line_native[leg]["achieved_GBs"] = g
        line_native[leg]["frac_of_hbm_peak"] = g / HBM_PEAK_GBS
    for leg, kern in (("match", "fm_match_kernel<dimer>"), ("locate", "fm_locate_kernel<dimer>")):
        t = measured_traffic(kern)
        if t:
            line_native[leg]["traffic"] = t
    return {"genome_symbols": ng, "index_build_s": build_s, "seeds": a.seeds, "seed_len": 22,
            "match": {"kernel": "fm_match_kernel", "kernel_ms": match_ms, "Mseeds_per_s": a.seeds / (match_ms * 1e-3) / 1e6,
                      "algorithmic_bytes_per_seed": bytes_per_seed, "achieved_GBs": mgbs, "frac_of_hbm_peak": mgbs / HBM_PEAK_GBS},
            "locate": {"kernel": "fm_locate_kernel", "rows": int(rows.numel()), "kernel_ms": locate_ms,
                       "Mrows_per_s": rows.numel() / (locate_ms * 1e-3) / 1e6, "mean_lf_steps": steps / mr,
                       "algorithmic_bytes_per_row": bytes_per_loc, "achieved_GBs": lgbs, "frac_of_hbm_peak": lgbs / HBM_PEAK_GBS,
                       "sorted_rows_kernel_ms": ref_sorted_ms},
            "line_native_index": line_native,
            "hbm_capacity_options": options,
            "parity": {"checked_seeds": m, "checked_rows": mr, "bit_exact": exact}}


def full_dp_leg(a, dev):
    """sw-benchmark's shape (sw-benchmark.cu:557-657): every read is aligned against the WHOLE reference
    with the full-matrix text-blocking Gotoh aligner, scoring (2,-1,-2,-1); 150-bp reads, one shared
    reference.  GCUPS = reads x read_len x ref_len / time, as sw-benchmark prints it (:380,441)."""
    import numpy as np
    from oracle import pyoracle as O
    n, L, N = a.full_reads, 150, a.full_ref
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED0006)
    ref = torch.randint(0, 4, (N,), dtype=torch.uint8, generator=g, device=dev)
    pos = torch.randint(0, N - L, (n,), generator=g, device=dev)
    sym = ref[pos.unsqueeze(1) + torch.arange(L, device=dev).unsqueeze(0)]
    sub = torch.rand((n, L), generator=g, device=dev) < 0.05
    sym = torch.where(sub, (sym + torch.randint(1, 4, (n, L), dtype=torch.uint8, generator=g, device=dev)) & 3, sym)
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    patterns = nvb.PackedStringSet(W._pack_chunked(sym.reshape(-1), 4, True), 4, True, idx * L, None, L)
    texts = nvb.PackedStringSet(W._pack_chunked(ref, 2, False), 2, False, torch.zeros(n, dtype=torch.int64, device=dev), None, N)
    res = {"reads": n, "read_len": L, "ref_len": N, "scheme": list(SCHEME)}
    score = torch.empty(n, dtype=torch.int32, device=dev)
    sink = torch.empty((n, 2), dtype=torch.int32, device=dev)
    for name, ty in (("local", nvb.LOCAL), ("semi_global", nvb.SEMI_GLOBAL), ("global", nvb.GLOBAL)):
        al = nvb.make_gotoh_aligner(ty, nvb.SimpleGotohScheme(*SCHEME))
        batch = nvb.BatchedAlignmentScore()
        batch.enact(al, patterns, texts, score, sink)
        torch.cuda.synchronize()
        reps = 3
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in evs:
            e0.record(); batch.enact(al, patterns, texts, score, sink); e1.record()
        torch.cuda.synchronize()
        ms = sum(e0.elapsed_time(e1) for e0, e1 in evs) / reps
        m = 256
        sub_p = nvb.PackedStringSet(patterns.words, 4, True, patterns.begin[:m].contiguous(), None, L)
        sub_t = nvb.PackedStringSet(texts.words, 2, False, texts.begin[:m].contiguous(), None, N)
        es, ek, _ = O.batch_gotoh_score(ty, SCHEME, O.StringSet.from_device(sub_p), O.StringSet.from_device(sub_t), n_threads=os.cpu_count() or 1)
        ok = bool((score[:m].cpu().numpy() == es).all() and (sink[:m].cpu().numpy().view(np.uint32) == ek).all())
        if not ok:
            raise SystemExit("parity gate failed: full-matrix Gotoh differs from the oracle")
        res[name] = {"kernel_ms": ms, "GCUPS": n * L * N / (ms * 1e-3) / 1e9, "Mreads_per_s": n / (ms * 1e-3) / 1e6, "parity_checked": m, "bit_exact": ok,
                     "kernel": nvb.lib().nvbio_hip_last_kernel().decode()}
        # roofline of the full-matrix sweep: integer-VALU issue.  `frac` is the EXECUTED lane-op rate (SQ_INSTS_VALU x 64 of the committed PMC pass
        # of this command, per cell, x the cells of this run) against the VALU lane-op peak -- a fraction of what the SIMDs can issue, never above 1.
        # The nominal figure beside it counts the reference recurrence per alignment type (F, E, H: 6 adds + 3 max, substitution compare + select = 11
        # for GLOBAL; + the last-row report for SEMI_GLOBAL = 12; + max(.,0) and the sink compare / update for LOCAL = 14).
        cells = float(n) * L * N
        nominal = FULL_NOMINAL_OPS_PER_CELL[name]
        roof = {"bound": "valu", "peak": VALU_PEAK_TOPS, "unit": "T lane-op/s",
                "nominal": {"ops_per_cell": nominal, "achieved": cells * nominal / (ms * 1e-3) / 1e12, "frac": cells * nominal / (ms * 1e-3) / 1e12 / VALU_PEAK_TOPS}}
        try:
            with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
                pm = json.load(f).get("full_gotoh_score_kernel<%s>" % name)
        except Exception:
            pm = None
        if pm and pm.get("insts_valu_per_launch") and pm.get("cells_per_launch"):
            per_cell = pm["insts_valu_per_launch"] * 64.0 / pm["cells_per_launch"]
            roof.update({"achieved": per_cell * cells / (ms * 1e-3) / 1e12, "frac": per_cell * cells / (ms * 1e-3) / 1e12 / VALU_PEAK_TOPS,
                         "executed_lane_ops_per_cell": per_cell, "source": "SQ_INSTS_VALU, profiles/traffic.json", "counters_round": pm.get("round")})
        else:
            roof.update({"achieved": roof["nominal"]["achieved"], "frac": roof["nominal"]["frac"], "source": "nominal op count (no PMC pass committed)"})
        roof["counters"] = dp_counters("full_gotoh_score_kernel<%s>" % name)
        res[name]["roofline"] = roof
    # sw-benchmark's second leg (sw-benchmark.cu:641-657): the same reads, edit distance, SEMI_GLOBAL -- on the bit-vector kernel; "GCUPS" is
    # sw-benchmark's figure (matrix cells / time) although no matrix is filled
    al = nvb.make_edit_distance_aligner(nvb.SEMI_GLOBAL)
    ms = _timed(lambda: nvb.BatchedAlignmentScore().enact(al, patterns, texts, score, sink))
    m = 256
    sub_p = nvb.PackedStringSet(patterns.words, 4, True, patterns.begin[:m].contiguous(), None, L)
    sub_t = nvb.PackedStringSet(texts.words, 2, False, texts.begin[:m].contiguous(), None, N)
    es, ek = O.batch_sw_score(0, nvb.SEMI_GLOBAL, (0, -1, -1, -1), O.StringSet.from_device(sub_p), O.StringSet.from_device(sub_t))
    ok = bool((score[:m].cpu().numpy() == es).all() and (sink[:m].cpu().numpy().view(np.uint32) == ek).all())
    if not ok:
        raise SystemExit("parity gate failed: full-matrix edit distance differs from the oracle")
    res["edit_distance_semi_global"] = {"kernel": "edit_distance_bitvector_kernel", "kernel_ms": ms, "GCUPS": n * L * N / (ms * 1e-3) / 1e9,
                                        "Mreads_per_s": n / (ms * 1e-3) / 1e6, "parity_checked": m, "bit_exact": ok}
    return res


def compat_stream_leg(a, dev):
    """What the source-level drop-in route costs: ONE score stream of read VIEWS, the concept of nvBowtie's streams
    (alignment_utils.h:170-340 + score_best_inl.h:54-148 + scoring.h:206-356) -- tests/compat/nvbowtie_streams.hip: reads stored reversed and
    viewed through io::ReadLoader, quality strings, a quality-aware scheme, band 15, LOCAL -- enacted through BatchedBandedAlignmentScore
    (a) in place on the views (tuned-views: nvbio_hip_banded_gotoh_score_qual_views), (b) on the staged tuned route it replaced, (c) down the
    generic one-lane-per-job template.  Same hits, same outputs (compared), a sample against the oracle."""
    import ctypes as C
    import numpy as np
    from nvbio_amd import pipeline as P
    from oracle import pyoracle as O
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    path = os.path.join(ROOT, "tests", "compat", "libnvbowtie_streams.so")
    if not os.path.exists(path):
        return {"error": "tests/compat/libnvbowtie_streams.so is missing (python __graft_entry__.py builds it)"}
    from test_compat_nvbowtie_streams import Args, SCHEMES, scheme_tables
    lib = C.CDLL(path)
    lib.bt2_banded_score.argtypes = [C.POINTER(Args), C.c_char_p]
    lib.bt2_banded_score_generic.argtypes = [C.POINTER(Args)]
    lib.bt2_banded_score_staged.argtypes = [C.POINTER(Args), C.c_char_p]
    n, L, band, ng = min(a.reads, 10_000_000), READ_LEN, 15, 1 << 28
    g = torch.Generator(device=dev); g.manual_seed(0x5EED0011)
    text = torch.randint(0, 4, (ng,), dtype=torch.uint8, generator=g, device=dev)
    sym, pos, is_rc = P.make_reads(text, n, L, seed=0x5EED0012)
    genome_words = W._pack_chunked(text, 2, True)
    rev_words = W._pack_chunked(sym.flip(1).reshape(-1), 4, True)                     # nvBowtie stores reads reversed
    quals = torch.randint(0, 60, (n * L + 8,), dtype=torch.uint8, generator=g, device=dev)
    index = (torch.arange(n + 1, dtype=torch.int64, device=dev) * L).to(torch.int32)
    hits = torch.stack([torch.arange(n, dtype=torch.int64, device=dev), pos, is_rc.to(torch.int64)], dim=1).to(torch.int32).contiguous()
    idx_queue = torch.arange(n, dtype=torch.int32, device=dev)
    second = torch.full((n,), -40, dtype=torch.int32, device=dev)
    out = {k: torch.zeros(n if k != "raw_sink" else (n, 2), dtype=torch.int32, device=dev) for k in ("hit_score", "hit_sink", "raw_score", "raw_sink")}
    args = Args()
    (args.rdg_c, args.rdg_k, args.rfg_c, args.rfg_k, args.match, args.mmp_min, args.mmp_max, args.local) = SCHEMES["local"]
    args.band_len = band
    args.read_words, args.read_quals, args.read_index, args.longest = rev_words.data_ptr(), quals.data_ptr(), index.data_ptr(), L
    args.mate_words, args.mate_quals, args.mate_index, args.mate_longest = rev_words.data_ptr(), quals.data_ptr(), index.data_ptr(), L
    args.genome_words, args.genome_length = genome_words.data_ptr(), ng
    args.idx_queue, args.hits, args.n_hits = idx_queue.data_ptr(), hits.data_ptr(), n
    args.second_best, args.score_limit = second.data_ptr(), -40
    for k, t in out.items():
        setattr(args, k, t.data_ptr())
    pathbuf = C.create_string_buffer(16)

    def timed(fn, reps=3):
        fn(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    def tuned():
        if lib.bt2_banded_score(C.byref(args), pathbuf) != 0:
            raise SystemExit("compat stream leg: bt2_banded_score failed")

    def generic():
        if lib.bt2_banded_score_generic(C.byref(args)) != 0:
            raise SystemExit("compat stream leg: bt2_banded_score_generic failed")

    ms_t = timed(tuned)
    route = pathbuf.value.decode()
    ts, tk = out["raw_score"].clone(), out["raw_sink"].clone()
    out["raw_score"].zero_(); out["raw_sink"].zero_()

    def staged():
        if lib.bt2_banded_score_staged(C.byref(args), pathbuf) != 0:
            raise SystemExit("compat stream leg: bt2_banded_score_staged failed")

    ms_s = timed(staged)
    same_s = bool(torch.equal(ts, out["raw_score"]) and torch.equal(tk, out["raw_sink"]))
    out["raw_score"].zero_(); out["raw_sink"].zero_()
    ms_g = timed(generic, reps=1)
    same = bool(same_s and torch.equal(ts, out["raw_score"]) and torch.equal(tk, out["raw_sink"]))
    # a sample against the oracle
    m = 20000
    lut, s5, ty = scheme_tables(SCHEMES["local"])
    comp = np.array([3, 2, 1, 0, 4], np.uint8)
    hs, hq = sym[:m].cpu().numpy(), quals[: m * L].cpu().numpy().reshape(m, L)[:, ::-1]        # forward reads, forward qualities
    rc = is_rc[:m].cpu().numpy()
    pats = [comp[hs[i]][::-1] if rc[i] else hs[i] for i in range(m)]
    qs = [hq[i][::-1] if rc[i] else hq[i] for i in range(m)]
    ps = O.StringSet.from_lists(pats, 4, True)
    qbuf = np.concatenate(qs + [np.zeros(8, np.uint8)])
    hp = pos[:m].cpu().numpy()
    gb = np.where(hp > band // 2, hp - band // 2, 0)
    tset = O.StringSet(genome_words[: (int(gb.max()) + L + band) // 16 + 4].cpu().numpy().view(np.uint32), 2, True, gb.astype(np.uint64),
                       (np.minimum(gb + band + L, ng) - gb).astype(np.uint32))
    es, ek = O.batch_banded_gotoh_score_qual(band, ty, s5 + (0,), lut, qbuf, ps, tset)
    ok = bool((ts[:m].cpu().numpy() == es).all() and (tk[:m].cpu().numpy().view(np.uint32) == ek).all())
    if not (same and ok):
        raise SystemExit("parity gate failed: compat stream routes disagree (tuned vs generic %s, tuned vs oracle %s)" % (same, ok))
    return {"stream": "nvBowtie-shaped BestScoreStream (ReadLoader views of reversed reads, quality strings, SmithWatermanScoringScheme), band 15, LOCAL, %d hits x %d bp" % (n, L),
            "tuned_route": {"path": route, "ms_per_enact": ms_t, "Mreads_per_s": n / ms_t / 1e3,
                            "includes": "job-description kernel (the stream's own init_context / load_strings, one lane per job: where the stored read lies and how it is viewed), one host sync, the tuned kernel reading the stored reads in place through their views, the stream's output()"},
            "staged_route": {"ms_per_enact": ms_s, "Mreads_per_s": n / ms_s / 1e3, "note": "the r03 route: patterns and qualities copied to a scratch by sixteen lanes per job first"},
            "generic_lane": {"ms_per_enact": ms_g, "Mreads_per_s": n / ms_g / 1e3},
            "identical_outputs": same, "oracle_sample": {"checked": m, "bit_exact": ok}}


def _timed(fn, reps=3):
    fn(); torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in evs:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return sum(e0.elapsed_time(e1) for e0, e1 in evs) / reps


def extras_leg(a, dev):
    """Throughput of the kernels built around the hot path: banded traceback -> CIGAR, the
    one-mismatch seed mappers, edit-distance full-matrix scoring (sw-benchmark's second leg), score reduction
    + MAPQ, and the composed single-end aligner.  Each with a sample checked exactly against the oracle.
    Opt-in (`--only extras`): not part of the default line."""
    import numpy as np
    from oracle import pyoracle as O
    from nvbio_amd import pipeline as P
    out = {}
    # ---- banded traceback, 100 bp x band 15 LOCAL (the read shape of config 2)
    n = 2_000_000
    p, t = W.make_sw_batch(n, READ_LEN, REF_LEN, seed=0x5EED0005, device=dev)
    al = nvb.make_gotoh_aligner(nvb.LOCAL, nvb.SimpleGotohScheme(*SCHEME))
    tb = nvb.BatchedBandedAlignmentTraceback(BAND)
    o = dict(score=torch.empty(n, dtype=torch.int32, device=dev), sink=torch.empty((n, 2), dtype=torch.int32, device=dev),
             source=torch.empty((n, 2), dtype=torch.int32, device=dev), cigar=torch.zeros((n, 32), dtype=torch.int16, device=dev),
             cigar_len=torch.empty(n, dtype=torch.int32, device=dev))
    temp = torch.empty(tb.min_temp_storage(READ_LEN, 0, n), dtype=torch.uint8, device=dev)
    ms = _timed(lambda: tb.enact(al, p, t, o["score"], o["sink"], o["source"], o["cigar"], o["cigar_len"], temp=temp))
    m = 20_000
    sub = lambda s_: O.StringSet(s_.words, s_.bits, s_.big_endian, s_.begin[:m], s_.length[:m])
    e = O.batch_banded_gotoh_traceback(BAND, O.LOCAL, SCHEME, sub(O.StringSet.from_device(p)), sub(O.StringSet.from_device(t)), 32)
    ok = all(bool((o[k][:m].cpu().numpy().view(e[k].dtype) == e[k]).all()) for k in ("score", "sink", "source", "cigar_len", "cigar"))
    out["banded_traceback"] = {"alignments": n, "kernel_ms": ms, "Malignments_per_s": n / ms / 1e3, "flag_bytes_per_alignment": READ_LEN * 8,
                               "flag_GBs_write_plus_read": 2 * n * READ_LEN * 8 / (ms * 1e-3) / 1e9, "parity_checked": m, "bit_exact": ok}
    del p, t, o, temp
    # ---- edit distance, full matrix, SEMI_GLOBAL (sw-benchmark.cu:641-657)
    nr, ref_len = 65536, 16384
    g = torch.Generator(device=dev); g.manual_seed(0x5EED0006)
    ref = torch.randint(0, 4, (ref_len,), dtype=torch.uint8, generator=g, device=dev)
    st = torch.randint(0, ref_len - 150, (nr,), generator=g, device=dev)
    reads = ref[st.unsqueeze(1) + torch.arange(150, device=dev).unsqueeze(0)]
    mut = torch.rand((nr, 150), generator=g, device=dev) < 0.04
    reads = torch.where(mut, (reads + 1) & 3, reads)
    rp = nvb.PackedStringSet(W._pack_chunked(reads.reshape(-1), 4, True), 4, True, torch.arange(nr, dtype=torch.int64, device=dev) * 150, None, 150)
    rt = nvb.PackedStringSet(W._pack_chunked(ref, 2, False), 2, False, torch.zeros(nr, dtype=torch.int64, device=dev), None, ref_len)
    ed = nvb.make_edit_distance_aligner(nvb.SEMI_GLOBAL)
    ms = _timed(lambda: nvb.batch_alignment_score(ed, rp, rt, 150, ref_len))
    gs, gk, _ = nvb.batch_alignment_score(ed, rp, rt, 150, ref_len)
    m = 256
    hp, ht = O.StringSet.from_device(rp), O.StringSet.from_device(rt)
    es, ek = O.batch_sw_score(0, O.SEMI_GLOBAL, (0, -1, -1, -1), O.StringSet(hp.words, 4, True, hp.begin[:m], hp.length[:m]), O.StringSet(ht.words, 2, False, ht.begin[:m], ht.length[:m]))
    ok = bool((gs[:m].cpu().numpy() == es).all() and (gk[:m].cpu().numpy().view(np.uint32) == ek).all())
    out["edit_distance_full"] = {"reads": nr, "read_len": 150, "ref_len": ref_len, "kernel_ms": ms, "GCUPS": nr * 150 * ref_len / ms / 1e6, "parity_checked": m, "bit_exact": ok}
    del rp, rt, reads
    # ---- the two extension kernels at the paired-end shape of BASELINE config 5: 2 x 150 bp, LOCAL, band 31
    # anchor mate: banded LOCAL band 31 with nvBowtie's quality-aware local scheme; opposite mate: full-matrix LOCAL
    # of the 150-bp mate against a 650-bp insert window with a min_score (score_opposite_inl.h:266)
    n = 4_000_000
    p, t = W.make_sw_batch(n, 150, 150 + 31, seed=0x5EED0007, device=dev)
    q = torch.randint(2, 41, (n * 150 + 8,), dtype=torch.uint8, generator=g, device=dev)
    loc = nvb.SmithWatermanScoringScheme.local()
    al31 = nvb.make_gotoh_aligner(nvb.LOCAL, loc)
    sc31 = torch.empty(n, dtype=torch.int32, device=dev); sk31 = torch.empty((n, 2), dtype=torch.int32, device=dev)
    b31 = nvb.BatchedBandedAlignmentScore(31)
    ms = _timed(lambda: b31.enact(al31, p, t, sc31, sk31, quals=q))
    m = 20_000
    st = loc.struct()
    lut = np.array([st.mismatch[k] for k in range(256)], dtype=np.int32)
    s6 = (st.match, st.pattern_gap_open, st.pattern_gap_ext, st.text_gap_open, st.text_gap_ext, 0)
    hp, ht = O.StringSet.from_device(p), O.StringSet.from_device(t)
    es, ek = O.batch_banded_gotoh_score_qual(31, O.LOCAL, s6, lut, q.cpu().numpy(), O.StringSet(hp.words, 4, True, hp.begin[:m], hp.length[:m]),
                                             O.StringSet(ht.words, 2, False, ht.begin[:m], ht.length[:m]))
    ok = bool((sc31[:m].cpu().numpy() == es).all() and (sk31[:m].cpu().numpy().view(np.uint32) == ek).all())
    pe = {"anchor_banded_local_31": {"alignments": n, "read_len": 150, "kernel_ms": ms, "Malignments_per_s": n / ms / 1e3, "GCUPS": n * 150 * 31 / ms / 1e6,
                                     "kernel": nvb.lib().nvbio_hip_last_kernel().decode(), "parity_checked": m, "bit_exact": ok}}
    del p, t, q
    nw, wl = 1_000_000, 650
    g.manual_seed(0x5EED0008)
    win = torch.randint(0, 4, (nw, wl), dtype=torch.uint8, generator=g, device=dev)
    off = torch.randint(0, wl - 150, (nw,), generator=g, device=dev)
    mate = win.gather(1, off.unsqueeze(1) + torch.arange(150, device=dev).unsqueeze(0))
    mate = torch.where(torch.rand((nw, 150), generator=g, device=dev) < 0.04, (mate + 1) & 3, mate)
    mp_ = nvb.PackedStringSet(W._pack_chunked(mate.reshape(-1), 4, True), 4, True, torch.arange(nw, dtype=torch.int64, device=dev) * 150, None, 150)
    wt = nvb.PackedStringSet(W._pack_chunked(win.reshape(-1), 2, True), 2, True, torch.arange(nw, dtype=torch.int64, device=dev) * wl, None, wl)
    alo = nvb.make_gotoh_aligner(nvb.LOCAL, nvb.SimpleGotohScheme(2, -6, -8, -3), nvb.PATTERN_BLOCKING)      # nvBowtie's aligners carry the default tag
    msc = torch.full((nw,), 100, dtype=torch.int32, device=dev)
    ms = _timed(lambda: nvb.batch_alignment_score(alo, mp_, wt, 150, wl, msc))
    gs, gk, go = nvb.batch_alignment_score(alo, mp_, wt, 150, wl, msc)
    m = 2000
    hp, ht = O.StringSet.from_device(mp_), O.StringSet.from_device(wt)
    es, ek, eo = O.batch_score_pattern_blocking(0, O.LOCAL, (2, -6, -8, -3), O.StringSet(hp.words, 4, True, hp.begin[:m], hp.length[:m]),
                                                O.StringSet(ht.words, 2, True, ht.begin[:m], ht.length[:m]), min_score=np.full(m, 100, np.int32))
    ok = bool((gs[:m].cpu().numpy() == es).all() and (gk[:m].cpu().numpy().view(np.uint32) == ek).all() and (go[:m].cpu().numpy() == eo).all())
    pe["opposite_mate_full_local"] = {"pairs": nw, "mate_len": 150, "window": wl, "kernel_ms": ms, "Mpairs_per_s": nw / ms / 1e3, "GCUPS": nw * 150 * wl / ms / 1e6,
                                      "parity_checked": m, "bit_exact": ok}
    # opposite-mate traceback: full-matrix Gotoh traceback of the 150-bp mate in its 650-bp window
    ntb = 200_000
    tbp = nvb.PackedStringSet(mp_.words, 4, True, mp_.begin[:ntb].contiguous(), None, 150)
    tbt = nvb.PackedStringSet(wt.words, 2, True, wt.begin[:ntb].contiguous(), None, wl)
    ms = _timed(lambda: nvb.batch_alignment_traceback(alo, tbp, tbt, 150, wl, cigar_stride=32), reps=2)
    got = nvb.batch_alignment_traceback(alo, tbp, tbt, 150, wl, cigar_stride=32)
    m = 300
    e = O.batch_gotoh_traceback(O.LOCAL, (2, -6, -8, -3), O.StringSet(hp.words, 4, True, hp.begin[:m], hp.length[:m]), O.StringSet(ht.words, 2, True, ht.begin[:m], ht.length[:m]), 32)
    ok = all(bool((got[k][:m].cpu().numpy().view(e[k].dtype) == e[k][:m]).all()) for k in ("score", "sink", "source", "cigar_len", "cigar"))
    pe["opposite_mate_full_traceback"] = {"pairs": ntb, "kernel_ms": ms, "Mpairs_per_s": ntb / ms / 1e3, "flag_bytes_per_pair": ((150 + 7) // 8 + 1) * wl * 4,
                                          "parity_checked": m, "bit_exact": ok}
    out["paired_end_shapes"] = pe
    del win, mate, mp_, wt
    # ---- one-mismatch seed mappers + composed aligner on a forward + reverse index
    ng = int(min(a.genome, 1_000_000_000))
    g.manual_seed(0x5EED0003)
    text = torch.randint(0, 4, (ng,), dtype=torch.uint8, generator=g, device=dev)
    fmi = W.build_fm_index(text)
    rfmi = W.build_fm_index(text.flip(0).contiguous())
    nreads = 2_000_000
    sym, pos, _ = P.make_reads(text, nreads, READ_LEN, seed=0x5EED0004)
    reads_rev, ext_words = P.pack_read_streams(sym)
    mp = nvb.MappingParams()
    res = {}
    for name, kw in (("exact", dict(allow_sub=0)), ("approx_subseed12", dict(allow_sub=1, subseed_len=12)), ("case_pruning", dict(allow_sub=1, subseed_len=0))):
        ms = _timed(lambda: nvb.map_seeds(fmi, rfmi, reads_rev, mp, READ_LEN, hits_stride=64, **kw))
        h, c, _ = nvb.map_seeds(fmi, rfmi, reads_rev, mp, READ_LEN, hits_stride=64, **kw)
        res[name] = {"kernel_ms": ms, "Mreads_per_s": nreads / ms / 1e3, "seed_hits_per_read": float(c.float().mean().item())}
    m = 2000
    hostf = O.FMIndex(parts=(fmi.length, fmi.primary, np.array(fmi.L2, dtype=np.uint32), fmi.bwt_occ.cpu().numpy().view(np.uint32), fmi.ssa.cpu().numpy().view(np.uint32), fmi.sa_int))
    hostr = O.FMIndex(parts=(rfmi.length, rfmi.primary, np.array(rfmi.L2, dtype=np.uint32), rfmi.bwt_occ.cpu().numpy().view(np.uint32), rfmi.ssa.cpu().numpy().view(np.uint32), rfmi.sa_int))
    hr = O.StringSet.from_device(reads_rev)
    hr = O.StringSet(hr.words, 4, True, hr.begin[:m], hr.length[:m])
    sf = O.simple_func_table(2, 1.0, 1.15, READ_LEN + 1)
    pd = dict(seed_len=mp.seed_len, min_read_len=mp.min_read_len, max_hits=mp.max_hits, max_reseed=mp.max_reseed, retry=0, rep_seeds=mp.rep_seeds, fw=1, rc=1)
    eh, ec, _ = O.map_seeds(2, 0, hostf, hostr, hr, pd, sf, 64)
    gh, gc = h[:m].cpu().numpy().view(np.uint64), c[:m].cpu().numpy().view(np.uint32)
    ok = bool((gc == ec).all()) and all((np.sort(gh[r, :gc[r]]) == np.sort(eh[r, :ec[r]])).all() for r in range(m))
    res["parity"] = {"checked_reads": m, "algorithm": "case_pruning", "hit_sets_equal": ok}
    res["genome_symbols"] = ng; res["reads"] = nreads
    out["seed_mappers"] = res
    genome_words = W._pack_chunked(text, 2, True)
    be = P.HipBackend(fmi, None, mp, READ_LEN)
    ms = _timed(lambda: P.align_single_end(be, sym, genome_words, ng, packed=(reads_rev, ext_words)), reps=2)
    r = P.align_single_end(be, sym, genome_words, ng, packed=(reads_rev, ext_words))
    aligned = ((r["best"][0] >> 32) & 0xFFFFFFFF) != 0xFFFFFFFF
    at_true = (((r["best"][0] >> 32) & 0xFFFFFFFF) == torch.clamp(pos - BAND // 2, min=0)) & aligned
    out["align_single_end"] = {"reads": nreads, "ms_per_batch": ms, "Mreads_per_s": nreads / ms / 1e3, "extension_jobs": r["n_jobs"],
                               "aligned": float(aligned.float().mean().item()), "best_at_true_position": float(at_true.float().mean().item()),
                               "mapq_ge_23": float((r["mapq"] >= 23).float().mean().item()),
                               "stages": "map_exact, locate, banded extend, score_reduce, BowtieMapq2, banded traceback (glue in torch)"}
    # ---- the same batch through nvBowtie's own single-end driver (Aligner::best_approx): seeding passes, randomized hit
    # selection, locate, quality-aware banded extension (band 31 = band_length(max_dist 15)), reduction with give-up counters,
    # re-seeding, MAPQ, traceback
    from nvbio_amd import aligner as AL, select as SEL
    names = SEL.pack_names(["r%d" % i for i in range(nreads)], dev)
    ba = {}
    for cname, kw in (("default", dict()), ("no_rand", dict(randomized=False)), ("one_mismatch_seeds", dict(allow_sub=1))):
        prm = AL.Params(hits_stride=16 if not kw.get("allow_sub") else 64, batch_size=nreads, **kw)
        run = lambda st=False: AL.best_approx(fmi, rfmi, sym, genome_words, ng, prm, names=names, packed=(reads_rev, ext_words), stage_times=st)
        ms = _timed(run, reps=2)
        r = run(True)
        loc = (r["best"][0] >> 32) & 0xFFFFFFFF
        aligned = loc != 0xFFFFFFFF
        at_true = aligned & ((loc - pos).abs() <= 2)
        ba[cname] = {"reads": nreads, "ms_per_batch": ms, "Mreads_per_s": nreads / ms / 1e3, "extensions": r["stats"]["extensions"], "dp_jobs": r.get("dp_jobs"),
                     "rounds": r["stats"]["rounds"], "queue_per_seeding_pass": r["stats"]["queue"],
                     "aligned": float(aligned.float().mean().item()), "best_at_true_position": float(at_true.float().mean().item()),
                     "mapq_ge_23": float((r["mapq"] >= 23).float().mean().item()),
                     "stage_ms": {k: round(v, 3) for k, v in r["stats"]["ms"].items()}}
    # parity of the composed driver on a sample: the first 2000 reads as their own batch vs the numpy driver over the oracle
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests"))
    import oracle_driver as OD
    m = 2000
    prm = AL.Params(hits_stride=16, batch_size=m)
    nm = ["r%d" % i for i in range(m)]
    rs = AL.best_approx(fmi, rfmi, sym[:m].contiguous(), genome_words, ng, prm, names=nm, cigar_stride=64)
    es = OD.best_approx(hostf, hostr, sym[:m].cpu().numpy(), genome_words.cpu().numpy().view(np.uint32), ng, prm, nvb.SmithWatermanScoringScheme(), nm, 2)
    ids = rs["aligned_ids"].cpu().numpy()
    ok = bool((rs["best"].cpu().numpy().view(np.uint64) == es["best"]).all() and (rs["mapq"].cpu().numpy() == es["mapq"]).all()
              and (rs["cigar"].cpu().numpy()[ids].view(np.uint16) == es["tb"]["cigar"][: ids.size]).all() and rs["stats"] == es["stats"])
    ba["parity"] = {"checked_reads": m, "best_mapq_cigar_stats_equal": ok}
    ba["stages"] = "per seeding pass: map -> select_init -> rounds of {select, locate, banded extend (quality-aware scheme), score_reduce + give-up counters}; mark_unaligned / re-seed queue; BowtieMapq2; banded traceback"
    out["best_approx_single_end"] = ba
    # ---- the same reads through nvBowtie's all-mapping driver (Aligner::all): every row of every seed hit range located,
    # de-duplicated per batch of BATCH_SIZE hits, extended, accepted at min_score(read_len), traced back, finished
    am = {}
    prm = AL.Params(hits_stride=16, batch_size=1 << 22)
    run = lambda st=False: AL.all_mapping(fmi, rfmi, sym, genome_words, ng, prm, packed=(reads_rev, ext_words), stage_times=st)
    ms = _timed(run, reps=2)
    r = run(True)
    n_aln = int(r["read_id"].numel())
    first = torch.zeros(nreads, dtype=torch.bool, device=dev); first[r["read_id"].long()] = True
    at = torch.zeros(nreads, dtype=torch.bool, device=dev)
    at[r["read_id"].long()[((((r["alignments_scored"] >> 32) & 0xFFFFFFFF) - pos[r["read_id"].long()]).abs() <= 2)]] = True
    am["default"] = {"reads": nreads, "ms_per_batch": ms, "Mreads_per_s": nreads / ms / 1e3, "seed_hit_rows": r["stats"]["hits"], "unique_placements": r["stats"]["unique"],
                     "alignments": n_aln, "Malignments_per_s": n_aln / ms / 1e3, "reads_with_alignment": float(first.float().mean().item()),
                     "true_position_reported": float(at.float().mean().item()), "stage_ms": {k: round(v, 3) for k, v in r["stats"]["ms"].items()}}
    m = 1500
    prm = AL.Params(hits_stride=16, batch_size=4096)
    rs = AL.all_mapping(fmi, rfmi, sym[:m].contiguous(), genome_words, ng, prm, cigar_stride=64)
    es = OD.all_mapping(hostf, hostr, sym[:m].cpu().numpy(), genome_words.cpu().numpy().view(np.uint32), ng, prm, nvb.SmithWatermanScoringScheme(), 2)
    k = es["read_id"].size
    ok = bool(rs["stats"] == es["stats"] and rs["read_id"].numel() == k and (rs["read_id"].cpu().numpy().view(np.uint32) == es["read_id"]).all()
              and (rs["alignments"].cpu().numpy().view(np.uint64) == es["alignments"]).all()
              and (rs["cigar"].cpu().numpy().view(np.uint16) == es["tb"]["cigar"][:k]).all()
              and (rs["mds_len"].cpu().numpy().view(np.uint32) == es["mds_len"]).all())
    am["parity"] = {"checked_reads": m, "alignments": int(k), "alignments_cigars_md_stats_equal": ok}
    am["stages"] = "map (all seeds, one pass) -> scans -> batches of {select_all, hi-bits sort, locate, (read, strand, position) sort, dedup + straddling marks, banded extend, accept at min_score}; banded traceback + finish_alignment of every accepted alignment"
    out["all_mapping_single_end"] = am
    # ---- BASELINE config 5 under nvBowtie's own paired-end driver: 2 x 150 bp FR pairs, --local (20-bp seeds, LOCAL band 31 in the
    # quality-aware local scheme), opposite mates by full-matrix DP in their fragment windows, paired reduction, discordant marking,
    # MAPQ per mate, anchor (banded) and opposite (full-matrix) tracebacks
    npairs = 500_000
    s1, s2, ppos, pflen = P.make_read_pairs(text, npairs, 150, seed=0x5EED0009)
    pnames = SEL.pack_names(["p%d" % i for i in range(npairs)], dev)
    bp = {}
    for cname, kw in (("local_default", dict(local=True, seed_len=20, seed_freq=(2, 1.0, 0.75))), ("end_to_end", dict())):
        prm = AL.Params(hits_stride=32, batch_size=npairs, **kw)
        run = lambda st=False: AL.best_approx_paired(fmi, rfmi, s1, s2, genome_words, ng, prm, names=pnames, stage_times=st)
        ms = _timed(run, reps=2)
        r = run(True)
        b0 = r["best"][0]
        paired = ((b0 >> 30) & 1) != 0
        conc = paired & (((b0 >> 31) & 1) == 0)
        a_pos = (b0 >> 32) & 0xFFFFFFFF
        ok_pos = (((a_pos - ppos).abs() <= 3) | ((a_pos - (ppos + pflen - 150)).abs() <= 3)) & conc
        bp[cname] = {"pairs": npairs, "ms_per_batch": ms, "Mpairs_per_s": npairs / ms / 1e3, "anchor_extensions": r["stats"]["extensions"], "opposite_dp_jobs": r.get("opposite_dp_jobs"),
                     "opposite_extensions": r["stats"]["opposite_extensions"], "rounds": r["stats"]["rounds"], "queue_per_seeding_pass": r["stats"]["queue"],
                     "concordant": float(conc.float().mean().item()), "concordant_at_fragment_end": float(ok_pos.float().mean().item()),
                     "mapq1_ge_23": float((r["mapq1"] >= 23).float().mean().item()), "stage_ms": {k: round(v, 3) for k, v in r["stats"]["ms"].items()}}
    m = 600
    prm = AL.Params(hits_stride=32, batch_size=m, local=True, seed_len=20, seed_freq=(2, 1.0, 0.75))
    nm = ["p%d" % i for i in range(m)]
    rs = AL.best_approx_paired(fmi, rfmi, s1[:m].contiguous(), s2[:m].contiguous(), genome_words, ng, prm, names=nm)
    es = OD.best_approx_paired(hostf, hostr, s1[:m].cpu().numpy(), s2[:m].cpu().numpy(), genome_words.cpu().numpy().view(np.uint32), ng, prm,
                               nvb.SmithWatermanScoringScheme.local(), nm, 1)
    ok = bool(all((rs[k].cpu().numpy().view(np.uint64) == es[k]).all() for k in ("best", "best_o")) and (rs["mapq1"].cpu().numpy() == es["mapq1"]).all()
              and (rs["mapq2"].cpu().numpy() == es["mapq2"]).all() and rs["stats"] == es["stats"]
              and all((rs[sl]["cigar"].cpu().numpy().view(np.uint16) == es[sl]["cigar"]).all() for sl in ("tb1", "tb2")))
    bp["parity"] = {"checked_pairs": m, "best_mapq_cigar_stats_equal": ok}
    out["best_approx_paired_end"] = bp
    # ---- the same shape through the earlier stage composition (every located placement extended, no selection policy)
    mp20 = nvb.MappingParams(seed_len=20)                                    # nvBowtie --local: 20-bp seeds
    be2 = P.HipBackend(fmi, None, mp20, 150)
    ms = _timed(lambda: P.align_paired_end(be2, s1, s2, genome_words, ng), reps=2)
    r = P.align_paired_end(be2, s1, s2, genome_words, ng)
    paired = ((r["best"][0] >> 30) & 1) != 0
    a_pos = (r["best"][0] >> 32) & 0xFFFFFFFF
    ok_pos = (((a_pos - ppos).abs() <= 3) | ((a_pos - (ppos + pflen - 150)).abs() <= 3)) & paired
    out["align_paired_end"] = {"pairs": npairs, "ms_per_batch": ms, "Mpairs_per_s": npairs / ms / 1e3, "extension_jobs": r["n_jobs"], "opposite_mate_jobs": r["n_opposite"],
                               "paired": float(paired.float().mean().item()), "anchor_at_fragment_end": float(ok_pos.float().mean().item()),
                               "stages": "per anchor mate: map_exact, locate, banded LOCAL 31 (quality-aware), opposite windows, full-matrix LOCAL (pattern blocking, min_score), score_reduce_paired; then BowtieMapq2 paired (glue in torch)"}
    return out


def usable_cores():
    """Host cores this process may actually use: the cgroup CPU quota if there is one (the GPU boxes expose 256
    hardware threads but cap the container at 16 CPUs; running 256 threads under that cap is 2x slower than 16)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = max(1, min(n, int(int(quota) / int(period))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = max(1, min(n, q // per))
        except (OSError, ValueError):
            pass
    return n


def cpu_leg(a, patterns, texts):
    """The CPU oracle (the reference host path's arithmetic, OpenMP like HostThreadScheduler) on a
    bounded sample of the same workload, all host cores."""
    from oracle import pyoracle as O
    m = min(len(patterns), a.cpu_sample)
    sub_p = nvb.PackedStringSet(patterns.words, 4, True, patterns.begin[:m].contiguous(), None, READ_LEN)
    sub_t = nvb.PackedStringSet(texts.words, 2, False, texts.begin[:m].contiguous(), None, REF_LEN)
    hp, ht = O.StringSet.from_device(sub_p), O.StringSet.from_device(sub_t)
    cores = usable_cores()
    O.batch_banded_gotoh_score(BAND, O.LOCAL, SCHEME, hp, ht, n_threads=cores, native=True)      # warm-up
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        es, ek = O.batch_banded_gotoh_score(BAND, O.LOCAL, SCHEME, hp, ht, n_threads=cores, native=True)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    # the whole sample doubles as the full-size parity check of BASELINE config 2: every score and sink
    import numpy as np
    gs, gk = nvb.batch_banded_alignment_score(BAND, nvb.make_gotoh_aligner(nvb.LOCAL, nvb.SimpleGotohScheme(*SCHEME)), sub_p, sub_t)
    torch.cuda.synchronize()
    exact = bool((gs.cpu().numpy() == es).all() and (gk.cpu().numpy().view(np.uint32) == ek).all())
    if not exact:
        raise SystemExit("parity gate failed: HIP scores differ from the oracle on the CPU-baseline sample")
    # the drop-in layer's own host execution (HostThreadScheduler: the per-job template under OpenMP, nvbio_hip_banded_gotoh_score_host)
    # on the same sample and threads
    twin = None
    try:
        import ctypes as C
        from nvbio_amd import _lib

        def sset(hs):
            ss = _lib.StringSetStruct()
            ss.words, ss.n_words, ss.bits, ss.big_endian = hs.words.ctypes.data, hs.words.size, hs.bits, hs.big_endian
            ss.begin, ss.length, ss.fixed_length = hs.begin.ctypes.data, hs.length.ctypes.data, 0
            return ss
        sp_, st_ = sset(hp), sset(ht)
        hs_, hk_ = np.zeros(m, np.int32), np.zeros((m, 2), np.uint32)
        gsch = _lib.GotohSchemeStruct(*SCHEME)
        tbest = None
        for _ in range(2):
            t0 = time.perf_counter()
            rc = nvb.lib().nvbio_hip_banded_gotoh_score_host(C.byref(gsch), int(O.LOCAL), BAND, C.byref(sp_), C.byref(st_), m, hs_.ctypes.data, hk_.ctypes.data, cores)
            dt = time.perf_counter() - t0
            tbest = dt if tbest is None else min(tbest, dt)
        twin = {"value": m / tbest, "unit": "reads/s", "threads": cores, "bit_exact_vs_oracle": bool(rc == 0 and (hs_ == es).all() and (hk_ == ek).all())}
    except Exception as e:     # noqa: BLE001
        twin = {"error": str(e)}
    return {"value": m / best, "unit": "reads/s", "cores": cores, "host_physical_cores": physical_cores(), "host_hardware_threads": os.cpu_count(), "kind": "port",
            "host_scheduler_twin": twin,
            "sample": "%d of the same reads, band 15 LOCAL, OpenMP over jobs with %d threads (the container's CPU quota; the host has %d hardware threads), gcc -O3 -march=native, best of 3" % (m, cores, os.cpu_count() or 0),
            "gpu_vs_cpu_on_sample": {"compared": m, "bit_exact": exact}}


if __name__ == "__main__":
    main()
