#!/usr/bin/env python3
"""bench.py -- frames/s through voxelize -> sparse 3D backbone -> BEV head -> NMS on synthetic
160k-point Waymo-shape clouds (BASELINE.json config 2), one process per GPU.

  python bench.py --gpus N --steps K --warmup W
  (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...)

  python bench.py --gpus N alone (no launcher, WORLD_SIZE unset) starts the N ranks itself.
  Config 3 (train step, one RCCL gradient all-reduce per step):  python bench.py --mode train --gpus N

A step = one pass of the whole hot path over one batch of `--frames` resident point clouds per GPU.
Frames are sharded across ranks with NO data-path collective (forward-only inference shards by
frame: SURVEY 8e); RCCL is used only for the timing barrier / max-over-ranks. Inputs are already in
HBM when the timed region starts; each step ends with the one D2H of its final boxes / scores /
labels into host memory (inside the timed region; --device-results leaves them in HBM).

Prints ONE JSON line (rank 0) with the contract fields (metric, value, unit, higher_is_better, dtype, ms_per_step, ...). A plain run
does nothing else: set up, warm up, time --steps steps, write the last timed step's outputs if --dump-outputs DIR is given, print.
With --full the line also carries everything else the bench measures and checks:
  results_digest: every timed step's detections digested and compared with the same steps re-run on one stream (exit 1 if they differ)
  roofline     : the dominant conv kernel (today window_conv_f16_kernel<128>: split-fp16 on the fp16 MFMA pipe, priced against
                 2500 / 3 TFLOP/s) measured live with HIP events on the launch stream in a second pass right after the timed
                 region; `traffic` from the round's committed rocprofv3 --pmc passes of this same command
  cpu_baseline : the CPU oracle (oracle/, a port of the reference algorithm) timed on this box's host cores: median of five
                 full frames on all hardware threads, and one frame on ONE thread (rank 0, N = 1 only)
and, at N = 1 with --full unless --no-extras, measured in the same process right after the timed region (each its own engine, same clouds):
  value_fp32_mfma      frames/s of the same step with conv_math = "f32" (fp32-input MFMA everywhere: the reference's arithmetic)
  value_batch4         frames/s at the reference's eval batch (4 frames per step, voxel_rcnn_cproto_center.yaml:188)
  latency_1frame_ms    one frame per step
  module_api           frames/s of the same 48 frames through the drop-in modules (cpd_amd.models.CenterPoint, batch_dict API)
  train_step           config 3 on this GPU: ms per step / frames/s of CenterPointTrainer (forward + backward + Adam)
"""
import argparse
import json
import os
import re
import sys
import time

# A training process runs three streams per GPU (input-gradient chain, weight gradients, index chain); on HIP's default of four
# hardware queues per device two of them can share a queue and serialise (same box: 9.10 vs 8.80 ms per step). The inference runs keep
# the default (eight queues cost the 48-frame headline 2 %). Set before HIP initialises; an explicit GPU_MAX_HW_QUEUES wins.
if "--mode" in sys.argv and sys.argv[sys.argv.index("--mode") + 1:sys.argv.index("--mode") + 2] == ["train"]:
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from cpd_amd import dist_utils, ops  # noqa: E402
from cpd_amd.engine import CenterPointEngine, ModelConfig, init_state_dict  # noqa: E402
from cpd_amd.synthetic import waymo_cloud  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: dense fp32-input MFMA peak
PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA peak (no sparsity)
BF16X3_PRODUCTS = 6             # bf16 MFMA products per fp32 multiply-add in the split-bf16 kernels
F16X2_PRODUCTS = 3              # fp16 MFMA products per fp32 multiply-add in the split-fp16 kernels


def kernel_peak(kname):
    """fp32-equivalent matrix peak of a conv kernel: the split-bf16 kernels execute 6 bf16 products
    per algorithmic fp32 multiply-add, so their ceiling is the bf16 peak / 6."""
    if "bf16" in kname:
        return PEAK_BF16_MFMA_TFLOPS / BF16X3_PRODUCTS, "bf16 dense MFMA peak 2500 TFLOP/s / 6 partial products (split-bf16, fp32-level result)"
    if "f16" in kname:
        return PEAK_BF16_MFMA_TFLOPS / F16X2_PRODUCTS, "fp16 dense MFMA peak 2500 TFLOP/s / 3 partial products (split-fp16, fp32-level result)"
    return PEAK_FP32_MFMA_TFLOPS, "fp32-input MFMA peak"

POOL = 48                       # distinct synthetic frames per rank (seeds rank*48 .. rank*48+47: SURVEY 8d): every frame of the
                                # default 48-frame step is a different cloud (round 3 cycled 8 clouds six times)


def make_clouds(seeds, n_points):
    """the rank's synthetic clouds (numpy, host), generated on a few threads (numpy releases the GIL in its kernels)"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return list(ex.map(lambda s_: waymo_cloud(s_, n_points=n_points), seeds))


def kernel_source_hash():
    """BLAKE2 over the kernel sources (cpd_amd/csrc/*.hip, *.h, sorted): stamps which code a committed PMC pass measured"""
    import glob
    import hashlib
    h = hashlib.blake2b(digest_size=8)
    for f in sorted(glob.glob(os.path.join(REPO, "cpd_amd", "csrc", "*.hip")) + glob.glob(os.path.join(REPO, "cpd_amd", "csrc", "*.h"))):
        with open(f, "rb") as fh:
            h.update(os.path.basename(f).encode() + b"\0" + fh.read())
    return h.hexdigest()


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--frames", type=int, default=None, help="frames per step per GPU (default: 48 infer, 1 train)")
    ap.add_argument("--streams", type=int, default=2, help="batches in flight per GPU (worker threads, one HIP stream + engine "
                    "workspace each): the latency-bound sparse kernels of one batch overlap the matrix-bound dense ones of the other "
                    "(1 -> 2 streams: +3.2 %%, 3: +4.1 %%, profiles/README.md). The per-launch roofline pass always runs on ONE stream.")
    ap.add_argument("--points", type=int, default=160000)
    ap.add_argument("--full", action="store_true", help="besides the headline, everything else the bench measures and checks: the "
                    "roofline and hbm_stages passes, the results_digest check against a single-stream re-run, the N = 1 extras, the CPU "
                    "baseline (--mode train: the conv profile, the timed all-reduce and the cross-rank checks). Each of them can still be "
                    "switched off with its --no-* option. Off by default: a plain run sets up, warms up, times --steps steps and prints")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last timed step "
                    "returned as DIR/<name>.npy (float32; rank 0): infer = every frame's pred_boxes / pred_scores / pred_labels, "
                    "concatenated in frame order, and boxes_per_frame; train = loss, hm_loss, loc_loss and a fixed sample of the "
                    "updated parameters; over 64 MB in all, a fixed, seeded sample of the rows. Inputs are seeded: the same arguments give the "
                    "same inputs in every run")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the extra measurements the default N = 1 --full run appends to its line "
                    "(fp32-MFMA value, batch-4 and 1-frame figures, the config-3 train step)")
    ap.add_argument("--layers", action="store_true", help="print a per-launch table of the conv kernels (stderr; made by the per-launch profile pass of a --full run)")
    ap.add_argument("--row-order", choices=["bricks", "taps", "canonical"], default="taps",
                    help="internal row order of the strided sparse levels (ModelConfig.row_order)")
    ap.add_argument("--row-order-chunk", type=int, default=4096)
    ap.add_argument("--order-level0", type=int, choices=[0, 1], default=0, help="ModelConfig.row_order_level0")
    ap.add_argument("--plan-tile", type=int, choices=[128, 256], default=256, help="ModelConfig.plan_tile_rows")
    ap.add_argument("--plan", type=int, choices=[0, 1], default=0, help="--row-order bricks: plan the sub-manifold rulebooks of levels 2-4 "
                    "(ModelConfig.plan_rulebooks: the staged row-wave kernel)")
    ap.add_argument("--pair-rows", type=int, choices=[0, 1, 2], default=2, help="fp16-pair rows between the f16x2 sparse layers "
                    "(ModelConfig.pair_rows): 1 = levels 2-4, 2 = level 1 as well (pair_rows_level1)")
    ap.add_argument("--dense-pairs", type=int, choices=[0, 1], default=1, help="ModelConfig.pair_rows_dense: fp16-pair BEV / head maps between "
                    "the split-fp16 dense layers (round 5; 0 = fp32 dense maps, the round-4 form: same detections)")
    ap.add_argument("--index-stream", type=int, choices=[0, 1], default=1, help="ModelConfig.index_side_stream: the strided stages' index chain "
                    "(output sets, row order, rulebooks) on a second HIP stream, one stage ahead of the convolutions")
    ap.add_argument("--vox-batch-min", type=int, default=2, help="ModelConfig.batched_voxelizer_min_frames")
    ap.add_argument("--deblock-stream", type=int, choices=[0, 1], default=1, help="ModelConfig.deblock_side_stream: the first BEV deblock beside the "
                    "next level's convolutions, on the side stream")
    ap.add_argument("--dense-map", type=int, choices=[0, 1], default=1, help="ModelConfig.persistent_dense_map (0: densify into a fresh, fully "
                    "cleared map every step -- the round-4 form)")
    ap.add_argument("--conv-math", choices=["f16x2", "bf16x3", "f32"], default="f16x2",
                    help="arithmetic of the layers with >= 32 input channels: split-fp16 x2 (3 products) or split-bf16 x3 (6 products) "
                         "on the 16-bit matrix pipe (both fp32-level error), or fp32 MFMA")
    ap.add_argument("--host-input", action="store_true", help="points start in pinned HOST memory: the H2D copies are inside "
                    "the timed region (PCIe-inclusive rate; never the headline value)")
    ap.add_argument("--mode", choices=["infer", "train"], default="infer",
                    help="infer = BASELINE config 2 (the headline metric); train = config 3: forward + backward + "
                         "one RCCL gradient all-reduce + Adam, --frames (default 1) frames per GPU per step")
    ap.add_argument("--sync-bn", action="store_true", help="--mode train: SyncBatchNorm (the reference's --sync_bn, tools/train.py:32; off by "
                    "default there and here): BatchNorm statistics all-reduced over the ranks")
    ap.add_argument("--device-results", action="store_true", help="leave the final boxes on the device (default: the one D2H "
                    "of each step's boxes / scores / labels into host memory is inside the timed region, SURVEY 8d)")
    ap.add_argument("--api", choices=["engine", "modules"], default="engine",
                    help="engine = the fused CenterPointEngine (headline); modules = the drop-in module path: device voxelizer -> "
                         "batch_dict -> cpd_amd.models.CenterPoint (eval), spconv.install(conv_math=--conv-math)")
    ap.add_argument("--no-digest-check", action="store_true", help="--full: do not re-run steps on one stream to compare their "
                    "results_digest with the timed (multi-stream) steps'")
    ap.add_argument("--launch-check", action="store_true", help="only launch the --gpus ranks, rendezvous, run the timing "
                    "collectives (barrier, max over ranks) and print the n_gpus line: no GPU work (the CPU test of the N > 1 "
                    "launcher, backend from CPD_DIST_BACKEND)")
    args = ap.parse_args()
    if args.frames is None:
        args.frames = 48 if args.mode == "infer" else 1
    if not args.full:                 # a plain run: the headline alone
        args.no_cpu_baseline = args.no_roofline = args.no_extras = True
        if args.layers:
            print("bench.py: --layers prints the table of the per-launch profile pass, which runs with --full only: no table in this run",
                  file=sys.stderr)
    return args


DUMP_BYTES = 64 * 10 ** 6            # --dump-outputs: at most this many bytes on disk in all (.npy headers included)
NPY_HEADER = 128                      # bytes before the data of a .npy file of up to a few dimensions (numpy format 1.0)


def dump_outputs(out_dir, arrays):
    """--dump-outputs: {name: array} -> out_dir/<name>.npy, float32. Over DUMP_BYTES in all, every array of more than one row keeps
    a fixed, seeded sample of its rows, in order: arrays with the same number of rows keep the same rows (boxes and their scores stay
    paired), and a run with the same shapes keeps the same rows."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: np.ascontiguousarray(np.asarray(v, dtype=np.float32)) for k, v in arrays.items()}
    rows = {k: a.ndim > 0 and a.shape[0] > 1 for k, a in arrays.items()}            # arrays that can be cut down
    fixed = sum(a.nbytes for k, a in arrays.items() if not rows[k]) + NPY_HEADER * len(arrays)
    cut = sum(a.nbytes for k, a in arrays.items() if rows[k])
    if fixed > DUMP_BYTES:
        raise SystemExit("bench.py: --dump-outputs: the single-row outputs alone exceed %d bytes" % DUMP_BYTES)
    scale = min(1.0, (DUMP_BYTES - fixed) / cut) if cut else 1.0
    for name, a in sorted(arrays.items()):
        if rows[name] and scale < 1.0:
            keep = int(a.shape[0] * scale)                  # floor: the kept rows of all arrays fit the budget together
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def detection_arrays(results):
    """one step's per-frame detections -> {key: all frames' rows concatenated in frame order, boxes_per_frame}"""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    keys = sorted(results[0].keys()) if results else ["pred_boxes", "pred_labels", "pred_scores"]
    out = {k: np.concatenate([host(r[k]) for r in results]) if results else np.zeros((0,), np.float32) for k in keys}
    out["boxes_per_frame"] = np.array([host(r["pred_boxes"]).shape[0] for r in results])
    return out


class ConvProfiler:
    """Brackets every cpd_gather_conv launch with HIP events on the launch stream and books its
    ALGORITHMIC flops: 2 * (valid (row, tap) pairs) * c_in * c_out (padding / skipped taps excluded)."""

    def __init__(self):
        self.records = []
        self.pairs_cache = {}
        self._orig = None
        self.bytes_total = 0.0

    def _pairs(self, nbr, n_out, c_in=0, c_out=0):
        if nbr is None:
            return n_out
        # every step sees the same multiset of frames (B is a multiple of the pool), so a rulebook of a given
        # shape has the same pair count in every step: one reduction + read-back per layer, not per launch
        # (a level's strided-conv table and its SubM table have the same shape but different channel pairs)
        key = (tuple(nbr.shape), c_in, c_out)
        if key not in self.pairs_cache:
            self.pairs_cache[key] = int((nbr >= 0).sum().item())
        return self.pairs_cache[key]

    def __enter__(self):
        self._orig = ops.gather_conv
        prof = self

        def wrapped(inp, c_in, packed_w, nbr, kv, n_out, c_out, *a, **kw):
            kname = ops.gather_conv_tile(n_out, c_in, c_out, inp.stride(0), kw.get("dense", False), kw.get("bf16x3", False), nbr,
                                         math=kw.get("math"), scaled=kw.get("in_absmax") is not None, in_pairs=kw.get("in_pairs", False))
            pairs = prof._pairs(nbr, n_out, c_in, c_out)
            flops = 2.0 * pairs * c_in * c_out
            # algorithmic HBM bytes of the layer: every feature row once in and once out, the weights, the
            # residual when there is one, and -- sparse layers only -- 8 bytes per (input, output) pair of the rulebook
            dense = bool(kw.get("dense", False))
            res = kw.get("residual", a[2] if len(a) > 2 else None)
            nbytes = 4.0 * (inp.shape[0] * c_in + n_out * c_out) + 4.0 * kv * c_in * c_out + (0.0 if dense or nbr is None else 8.0 * pairs)
            if res is not None:
                nbytes += 4.0 * n_out * c_out
            prof.bytes_total += nbytes
            if kw.get("out") is None:          # allocate before the window: an allocator miss (hipMalloc) stalls the host,
                kw["out"] = torch.empty((n_out, c_out), dtype=torch.float32, device=inp.device)   # and the GPU idles meanwhile
            s = torch.cuda.current_stream()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with ops.launch_log() as log:          # the instantiation that actually ran (e.g. the f16pe form of a pair-row layer)
                e0.record(s)
                out = prof._orig(inp, c_in, packed_w, nbr, kv, n_out, c_out, *a, **kw)
                e1.record(s)
            ran = [k for k in log.counts if k != "split_finish_kernel"]
            if len(ran) == 1:
                kname = re.sub(r"^(window_conv_\w+_kernel<\d+),128>$", r"\1>", ran[0])     # (128-row window tiles: the short name)
            prof.records.append((kname, flops, e0, e1, (n_out, c_in, c_out, kv)))
            return out

        ops.gather_conv = wrapped
        return self

    def __exit__(self, *exc):
        ops.gather_conv = self._orig

    def summary(self):
        """kernel -> [flops, ms, launches]. Launches of one (kernel, layer shape) are priced at their MEDIAN
        duration: a window occasionally contains a host hiccup (allocator / runtime housekeeping with the GPU
        idle behind the start event) that is not kernel time -- rocprofv3's own averages confirm the medians."""
        torch.cuda.synchronize()
        groups = {}
        for key, flops, e0, e1, shp in self.records:
            groups.setdefault((key, shp), []).append((flops, e0.elapsed_time(e1)))
        agg = {}
        total_ms = 0.0
        for (key, _), items in groups.items():
            ts = sorted(t for _, t in items)
            med = ts[len(ts) // 2]
            a = agg.setdefault(key, [0.0, 0.0, 0])
            a[0] += sum(f for f, _ in items)
            a[1] += med * len(items)
            a[2] += len(items)
            total_ms += med * len(items)
        return agg, total_ms


class HbmStageProfiler:
    """HIP-event timing of the HBM-bound stages with their ALGORITHMIC bytes: voxelizer + fused
    MeanVFE, rulebook builds, the 5/16-channel sparse convs, densify. Reported next to the HBM roofline
    (8 TB/s nominal, MI355X_MICROARCH.md); the matrix-bound conv kernels are `roofline` proper."""

    def __init__(self):
        self.rec = {}
        self._undo = []

    def _add(self, name, nbytes, e0, e1):
        self.rec.setdefault(name, []).append((nbytes, e0, e1))

    def _wrap(self, obj, attr, name, bytes_fn):
        orig = getattr(obj, attr)
        prof = self

        def wrapped(*a, **kw):
            s = torch.cuda.current_stream()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            out = orig(*a, **kw)
            e1.record(s)
            prof._add(name, (a, kw, out, bytes_fn), e0, e1)
            return out

        setattr(obj, attr, wrapped)
        self._undo.append((obj, attr, orig))

    def __enter__(self):
        # 4*N*C read + 4*M*(C+4+1) write (M resolved after the run from the device counter)
        self._wrap(ops.Voxelizer, "__call__", "voxelize+mean_vfe",
                   lambda a, kw, out: 4.0 * a[1].shape[0] * a[1].shape[1] + 4.0 * float(out[4].item()) * (a[1].shape[1] + 5))
        self._wrap(ops.Voxelizer, "batch", "voxelize+mean_vfe",
                   lambda a, kw, out: sum(4.0 * p.shape[0] * p.shape[1] for p in a[1]) +
                   4.0 * float(out[4][-1].item()) * (a[1][0].shape[1] + 5))
        # rulebook: read 16*N_in, write the kv x N_out table (4 B per entry) + tap masks
        self._wrap(ops, "rulebook_subm", "rulebook_subm", lambda a, kw, out: 16.0 * a[0].shape[0] + 4.0 * out.numel())
        self._wrap(ops, "rulebook_conv", "rulebook_conv", lambda a, kw, out: 16.0 * a[0].shape[0] + 4.0 * out.numel())
        self._wrap(ops, "densify_nhwc", "densify", lambda a, kw, out: 4.0 * a[0].numel() + 4.0 * out.numel())
        orig = ops.gather_conv
        prof = self

        def conv(inp, c_in, packed_w, nbr, kv, n_out, c_out, *a, **kw):
            if c_in > 16 or kw.get("dense", False):
                return orig(inp, c_in, packed_w, nbr, kv, n_out, c_out, *a, **kw)
            s = torch.cuda.current_stream()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            out = orig(inp, c_in, packed_w, nbr, kv, n_out, c_out, *a, **kw)
            e1.record(s)
            pairs = int((nbr >= 0).sum().item()) if nbr is not None else n_out
            nb = 4.0 * (inp.shape[0] * c_in + n_out * c_out) + 4.0 * kv * c_in * c_out + 8.0 * pairs
            prof._add("sparse_conv_c<=16", (None, None, None, lambda *_: nb), e0, e1)
            return out

        ops.gather_conv = conv
        self._undo.append((ops, "gather_conv", orig))
        return self

    def __exit__(self, *exc):
        for obj, attr, orig in reversed(self._undo):
            setattr(obj, attr, orig)

    def summary(self, frames, peak_gbps=8000.0):
        torch.cuda.synchronize()
        out = {}
        for name, items in self.rec.items():
            nbytes = sum(fn(a, kw, o) for (a, kw, o, fn), _, _ in items)
            ms = sum(e0.elapsed_time(e1) for _, e0, e1 in items)
            out[name] = {"us_per_frame": 1e3 * ms / frames, "algorithmic_MB_per_frame": nbytes / frames / 1e6,
                         "GBps": nbytes / (ms * 1e-3) / 1e9, "frac_of_hbm_peak": nbytes / (ms * 1e-3) / 1e9 / peak_gbps,
                         "launch_groups_per_frame": len(items) / frames}
        return out


def pmc_summary_file():
    """the newest committed PMC summary (profiles/rNN_pmc_summary.json, written by tools/pmc_bench.sh from this command)"""
    import glob
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "r[0-9][0-9]_pmc_summary.json")))
    return files[-1] if files else None


def pmc_traffic(kernel):
    """HBM-side bytes per launch of `kernel` from the round's committed rocprofv3 PMC passes of this command
    (2 x FETCH_SIZE + WRITE_SIZE, per MI355X_MICROARCH.md), or None. bench.py cannot run the counters itself."""
    try:
        with open(pmc_summary_file()) as f:
            k = json.load(f)["kernels"].get(kernel)
        return k["hbm_bytes_per_launch_corrected"] if k else None
    except Exception:
        return None


def pmc_stamp():
    """which code the committed PMC passes measured: the git sha and kernel-source hash tools/pmc_bench.sh recorded in the summary,
    and whether the kernel sources of THIS run hash the same"""
    try:
        with open(pmc_summary_file()) as f:
            d = json.load(f)
        here = kernel_source_hash()
        return {"file": os.path.relpath(pmc_summary_file(), REPO), "git_sha": d.get("git_sha"),
                "kernel_source_hash": d.get("kernel_source_hash"), "this_run_kernel_source_hash": here,
                "same_kernel_sources": (d.get("kernel_source_hash") == here) if d.get("kernel_source_hash") else None}
    except Exception:
        return None


def mfma_power_probe(dev, seconds=1.2):
    """What the matrix pipe of THIS part sustains under its socket power cap (VERDICT r5 #3a): cpd_mfma_burn (csrc/diag.hip) -- waves of
    nothing but v_mfma_f32_16x16x32_f16 on register operands -- launched back to back for `seconds` per operand pattern on the current
    stream, HIP events around every group of launches, rocm-smi sampled alongside. Patterns: A post-ReLU-like (half zeros) x B random --
    what the dominant kernel multiplies (activations x weights) --, and random x random. -> dict for roofline["power_probe"]."""
    from cpd_amd._lib import check, lib, ptr, stream
    g = torch.Generator().manual_seed(3)
    rnd = lambda: (torch.randn(512 * 8, generator=g) * 1.5).half().to(dev)
    a_relu, b_rand, a_rand = torch.relu(rnd()), rnd(), rnd()
    blocks, iters = 256 * 8, 1500
    sink = torch.empty(blocks * 256, dtype=torch.float32, device=dev)
    flops = float(lib().cpd_mfma_burn_flops(blocks, iters))
    out = {}
    for name, a, b in (("relu_like_x_random", a_relu, b_rand), ("random_x_random", a_rand, b_rand)):
        launch = lambda: check(lib().cpd_mfma_burn(ptr(a), ptr(b), ptr(sink), blocks, iters, stream()), "cpd_mfma_burn")
        launch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:                       # let the clock settle under the load before the timed part
            launch()
            torch.cuda.synchronize()
        ms_total, n = 0.0, 0
        with ClockSampler() as clk:
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < seconds:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(5):
                    launch()
                e1.record()
                e1.synchronize()
                ms_total += e0.elapsed_time(e1)
                n += 5
        cs = clk.summary()
        out[name] = {"f16_mfma_tflops": flops * n / (ms_total * 1e-3) / 1e12, "launches": n, "sclk_MHz_median": cs["sclk_MHz_median"],
                     "socket_power_W_median": cs["socket_power_W_median"]}
    return out


class ClockSampler:
    """rocm-smi (shader clock, socket power) sampled on a background thread while the block runs: the state the chip was in next to
    `roofline.frac` (the dominant kernel is limited by the socket power cap). Used around the single-stream roofline
    pass, never around the timed region."""

    def __enter__(self):
        import threading
        self.samples, self._stop = [], False

        def run():
            import subprocess
            while not self._stop:
                try:
                    o = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=5).stdout
                    d = json.loads(o)
                    c = d[sorted(d)[0]]
                    rec = {}
                    for k, v in c.items():
                        m = re.search(r"([0-9.]+)", str(v))
                        if not m:
                            continue
                        if "sclk" in k.lower() and "level" not in k.lower():         # ("sclk clock speed:": "(1910Mhz)"; the level key is an index)
                            rec["sclk_MHz"] = float(m.group(1))
                        elif "power" in k.lower() and "W" in k:
                            rec["power_W"] = float(m.group(1))
                    if rec:
                        if not self.samples:
                            rec["raw"] = {k: str(v) for k, v in c.items() if "sclk" in k.lower() or "power" in k.lower()}
                        self.samples.append(rec)
                except Exception:
                    pass
                time.sleep(0.2)
        self._t = threading.Thread(target=run, daemon=True)
        self._t.start()
        return self

    def __exit__(self, *exc):
        self._stop = True
        self._t.join(timeout=6)

    def summary(self):
        def med(key):
            v = sorted(x[key] for x in self.samples if key in x)
            return v[len(v) // 2] if v else None
        return {"samples": len(self.samples), "sclk_MHz_median": med("sclk_MHz"), "socket_power_W_median": med("power_W"),
                "first_sample_raw": self.samples[0].get("raw") if self.samples else None,
                "note": "rocm-smi sampled every ~0.2 s during the single-stream roofline pass (nominal peak clock 2400 MHz, socket cap 1400 W)"}


def time_steps(step, steps, warmup):
    """warmup + timed steps of step(i) on the current stream -> seconds per step"""
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(warmup + i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def module_api_runner(cfg, sd, dev, clouds, conv_math):
    """The drop-in module path on the same frames: the device voxelizer fills the reference's batch_dict keys
    (voxel_features -- MeanVFE fused --, voxel_coords, batch_size), cpd_amd.models.CenterPoint (reference class names, batch_dict
    contract, state_dict names) runs in eval mode under no_grad, results are copied to the host like the engine's."""
    from cpd_amd import models
    from cpd_amd import spconv as sp
    # (the engine's row order and -- round 6 -- its fast forms, both opt-in for modules: pair rows between fused sparse layers, the
    # optimistic range guard, the level-0 index the voxelizer built)
    sp.install(conv_math=conv_math, row_order="taps" if cfg.row_order == "taps" else "canonical", fast_eval=conv_math == "f16x2")
    net = models.CenterPoint(point_cloud_range=cfg.point_cloud_range, voxel_size=cfg.voxel_size).to(dev).eval()
    net.load_state_dict(sd)
    vox = ops.Voxelizer(cfg.voxel_size, cfg.point_cloud_range, cfg.num_point_features, cfg.max_points_per_voxel, cfg.max_voxels,
                        device=torch.device(dev))

    def run(frames):
        with torch.no_grad():
            _, coords, _, feats, nvox, index0 = vox.batch(frames, index_z_extra=1)
            n = int(nvox[len(frames)])
            bd = {"voxel_features": feats[:n], "voxel_coords": coords[:n], "batch_size": len(frames), "voxel_index": index0}
            preds, _ = net(bd)
            # results to the host: one concatenation + one copy per key (a blocking copy per frame and key -- 144 of them at 48
            # frames -- was 3 of the step's 55 ms spent in synchronisation), cut up again on the host
            keys = list(preds[0].keys())
            cnt = [int(p[keys[0]].shape[0]) for p in preds]
            host = {k: torch.cat([p[k] for p in preds]).cpu() for k in keys}
            out, o = [], 0
            for c in cnt:
                out.append({k: host[k][o:o + c] for k in keys})
                o += c
            return out

    return run


def extras(args, cfg, sd, dev, clouds, value, streams=()):
    """The extra figures of the default N = 1 line, each measured here with its own engine on the same clouds. `streams`: the HIP
    streams of the main run, re-used for the two-batches-in-flight figure (HIP deals streams to a few hardware queues in creation
    order; a fresh pair made after the main run's can land on ONE queue and serialise: 640 instead of 897 frames/s, round 3)."""
    out = {}
    B = args.frames

    def engine_rate(c, frames, steps, warmup, n_streams=1, host=None):
        """frames/s and seconds per step of `steps` steps of `frames` frames, dealt to n_streams workers (engine + HIP stream each).
        `host`: pinned host copies of the clouds -- the H2D copies then run inside the step, on the worker's stream"""
        import threading
        engs = [CenterPointEngine(c, sd, device=dev, host_results=not args.device_results) for _ in range(n_streams)]

        def batch_of(i):
            if host is not None:
                return [host[(i * frames + j) % POOL].cuda(non_blocking=True) for j in range(frames)]
            return [clouds[(i * frames + j) % POOL] for j in range(frames)]

        # host input, double-buffered: a worker's NEXT batch is copied on its own copy stream while the current one
        # computes; the compute stream waits on the copies' event only. (The voxelizer takes the frames where they land:
        # cpd_voxelize_batch_frames, no concatenation.)
        copy_streams = [torch.cuda.Stream(device=dev) for _ in range(n_streams)] if host is not None else []

        def prefetch(i, w):
            with torch.cuda.stream(copy_streams[w]):
                ts = [host[(i * frames + j) % POOL].cuda(non_blocking=True) for j in range(frames)]
                ev = copy_streams[w].record_event()
            return ts, ev

        def take(pending):
            ts, ev = pending
            cur = torch.cuda.current_stream()
            cur.wait_event(ev)
            for t in ts:
                t.record_stream(cur)
            return ts

        if n_streams == 1 and host is None:
            sec = time_steps(lambda i: engs[0].forward(batch_of(i)), steps, warmup)
            return frames / sec, sec
        strs = list(streams[:n_streams]) + [torch.cuda.Stream(device=dev) for _ in range(n_streams - len(streams))]

        def run(n):
            def worker(w):
                torch.cuda.set_device(torch.device(dev))
                with torch.cuda.stream(strs[w]):
                    if host is not None:
                        nxt = prefetch(w, w) if w < n else None
                        for i in range(w, n, n_streams):
                            cur = take(nxt)
                            nxt = prefetch(i + n_streams, w) if i + n_streams < n else None
                            engs[w].forward(cur)
                    else:
                        for i in range(w, n, n_streams):
                            engs[w].forward(batch_of(i))
                    strs[w].synchronize()
            ts = [threading.Thread(target=worker, args=(w,)) for w in range(n_streams)]
            [t.start() for t in ts]
            [t.join() for t in ts]

        run(warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        sec = (time.perf_counter() - t0) / steps
        return frames / sec, sec

    if cfg.conv_math != "f32":
        c32 = ModelConfig(conv_math="f32", row_order=cfg.row_order, row_order_chunk=cfg.row_order_chunk)
        v, sec = engine_rate(c32, B, 5, 2)
        out["value_fp32_mfma"] = {"value": v, "unit": "frames/s", "ms_per_step": 1e3 * sec, "steps": 5,
                                  "note": "same step with conv_math='f32': fp32-input MFMA (v_mfma_f32_16x16x4_f32) in every layer"}
    v, sec = engine_rate(cfg, 4, 40, 8)
    v2, sec2 = engine_rate(cfg, 4, 60, 8, n_streams=2)
    out["value_batch4"] = {"value": v, "unit": "frames/s", "ms_per_step": 1e3 * sec, "steps": 40,
                           "two_batches_in_flight": {"value": v2, "ms_per_step_amortised": 1e3 * sec2, "steps": 60},
                           "note": "4 frames per step: the reference's eval batch per GPU (voxel_rcnn_cproto_center.yaml:188); `value` = one "
                                   "stream (a step's latency = ms_per_step), two_batches_in_flight = two 4-frame batches on two HIP streams "
                                   "(three are slower: the host side of a 4-frame step is 3.6 ms of Python and the workers share the GIL)"}
    v, sec = engine_rate(cfg, 1, 60, 10)
    out["latency_1frame_ms"] = 1e3 * sec
    # the detector the shipped config actually selects (voxel_rcnn_cproto_center.yaml:13 NAME: VoxelRCNN): first stage as above, its NMS
    # output as RoIs -> RoI grid pooling on x_conv3 / x_conv4 -> shared FC / cls / reg GEMMs -> class-agnostic NMS 0.3, all on the
    # device (cpd_amd/two_stage.py). Random-init weights keep ~490 proposals per frame (a trained first stage keeps a few dozen): the
    # second stage here is at its most expensive.
    try:
        from cpd_amd import models
        from cpd_amd.two_stage import VoxelRCNNEngine
        mcfg = models.waymo_voxel_rcnn_cfg()
        torch.manual_seed(0)
        head_sd = {"roi_head." + k: v.detach().clone() for k, v in
                   models.__all__[mcfg.ROI_HEAD.NAME](input_channels={"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 128},
                                                      model_cfg=mcfg.ROI_HEAD, point_cloud_range=cfg.point_cloud_range,
                                                      voxel_size=cfg.voxel_size, num_class=1).state_dict().items()}
        two = VoxelRCNNEngine(cfg, mcfg.ROI_HEAD, mcfg.POST_PROCESSING, dict(sd, **head_sd), device=dev, host_results=not args.device_results)
        fb = min(B, 16)
        last, kept = [None], {}

        def two_step(i):                              # the production call: no intermediates (the pooled levels travel as fp16-pair rows)
            last[0] = two.forward([clouds[(i * fb + j) % POOL] for j in range(fb)])
            kept[i] = last[0]
        sec = time_steps(two_step, 4, 2)
        res = last[0]
        _, it = two.forward([clouds[j % POOL] for j in range(fb)], return_intermediates=True)       # (RoI count of the report; untimed)
        # results digest of the two-stage step (VERDICT r4 #2c), taken after the clock stopped: every timed step's final detections,
        # and the first timed step run once more -- the same frames must give bit-identical second-stage detections
        from cpd_amd.digest import step_digest
        dig = {i: step_digest(r) for i, r in sorted(kept.items()) if i >= 2}
        again = step_digest(two.forward([clouds[(2 * fb + j) % POOL] for j in range(fb)]))
        out["value_two_stage"] = {"value": fb / sec, "unit": "frames/s", "ms_per_step": 1e3 * sec, "steps": 4, "frames_per_step": fb,
                                  "results_digest": {"timed_steps": [dig[i][2] for i in sorted(dig)], "boxes_per_frame_step0": dig[2][0],
                                                     "step0_rerun": again[2], "repeatable": again[2] == dig[2][2]},
                                  "rois_per_frame": it["rois"].shape[1], "final_boxes_per_frame": sum(len(r["pred_boxes"]) for r in res) / fb,
                                  "note": "VoxelRCNN (two-stage) forward: CenterPoint proposals -> RoI grid pooling (6^3 grid, x_conv3 + x_conv4, two "
                                          "radii each) -> 27648->256->256 shared FC, cls / reg stacks -> final class-agnostic NMS 0.3; one stream"}
        del two
        torch.cuda.empty_cache()
    except Exception as e:                                # an extra must not take the headline line down
        out["value_two_stage"] = {"error": repr(e)[:300]}
    # the other shipped two-stage family (voxel_rcnn_dbscan / oyster_single_train.yaml): AnchorHeadSingleV2 proposals (6 anchors per BEV
    # cell, occupancy-masked, NMS 0.8 -> 200 RoIs per frame) -> VoxelRCNNHead -> NMS 0.3 (cpd_amd/anchor_engine.py + two_stage.py)
    try:
        from cpd_amd.anchor_engine import AnchorPointEngine, synthetic_two_stage_state
        from cpd_amd.two_stage import VoxelRCNNEngine
        mcfg, a_sd = synthetic_two_stage_state(cfg, sd, seed=1)
        rpn = AnchorPointEngine(cfg, a_sd, mcfg.DENSE_HEAD, mcfg.ROI_HEAD.NMS_CONFIG["TEST"], device=dev)
        two = VoxelRCNNEngine(cfg, mcfg.ROI_HEAD, mcfg.POST_PROCESSING, a_sd, device=dev, host_results=not args.device_results, rpn=rpn)
        fb = min(B, 16)
        last, kept = [None], {}

        def anchor_step(i):
            last[0] = two.forward([clouds[(i * fb + j) % POOL] for j in range(fb)])
            kept[i] = last[0]
        sec = time_steps(anchor_step, 4, 2)
        res = last[0]
        _, it = two.forward([clouds[j % POOL] for j in range(fb)], return_intermediates=True)
        # results digest, after the clock stopped: every timed step's final detections and the first timed step once more --
        # bit-identical or the figure is not printed as repeatable; the full-size parity test of this very model (same state dict builder)
        # is tests/test_gpu_two_stage.py::test_full_size_anchor_two_stage_engine_matches_the_oracle_composition
        from cpd_amd.digest import step_digest
        dig = {i: step_digest(r) for i, r in sorted(kept.items()) if i >= 2}
        again = step_digest(two.forward([clouds[(2 * fb + j) % POOL] for j in range(fb)]))
        out["value_two_stage_anchor"] = {"value": fb / sec, "unit": "frames/s", "ms_per_step": 1e3 * sec, "steps": 4, "frames_per_step": fb,
                                         "results_digest": {"timed_steps": [dig[i][2] for i in sorted(dig)], "boxes_per_frame_step0": dig[2][0],
                                                            "step0_rerun": again[2], "repeatable": again[2] == dig[2][2]},
                                         "proposal_full_reruns": int(getattr(rpn, "proposal_full_reruns", 0)),
                                         "rois_per_frame": it["rois"].shape[1], "anchors_per_frame": int(rpn.last_dense["batch_cls_preds"].shape[1]),
                                         "final_boxes_per_frame": sum(len(r["pred_boxes"]) for r in res) / fb,
                                         "note": "VoxelRCNN of the dbscan / oyster configs: AnchorHeadSingleV2 first stage (fp32 dense maps, occupancy-masked "
                                                 "anchors, proposal NMS 0.8 -> 200 RoIs) -> RoI grid pooling -> FC stacks -> final NMS 0.3; one stream"}
        del two, rpn
        torch.cuda.empty_cache()
    except Exception as e:
        out["value_two_stage_anchor"] = {"error": repr(e)[:300]}
    run = module_api_runner(cfg, sd, dev, clouds, cfg.conv_math)
    sec = time_steps(lambda i: run([clouds[(i * B + j) % POOL] for j in range(B)]), 6, 2)
    out["module_api"] = {"value": B / sec, "unit": "frames/s", "ms_per_step": 1e3 * sec, "steps": 6, "ratio_to_engine": B / sec / value,
                         "note": "device voxelizer -> batch_dict -> cpd_amd.models.CenterPoint (eval, no_grad; the row order of --row-order (tap-pattern by default: spconv.install(row_order=...)), "
                                 "fast eval (round 6: pair rows between fused sparse layers, optimistic range pass, the voxelizer's level-0 index; spconv.install(fast_eval=True)), "
                                 "first-appearance voxel order as at the B1 boundary), results copied to the host; ONE stream -- ratio_to_engine is "
                                 "against the headline's %d stream(s); two_batches_in_flight: two model instances on two HIP streams, as the headline runs" % max(1, args.streams)}
    if max(1, args.streams) >= 2:
        try:
            import threading
            runs = [run, module_api_runner(cfg, sd, dev, clouds, cfg.conv_math)]
            strs = list(streams[:2]) + [torch.cuda.Stream(device=dev) for _ in range(2 - len(streams[:2]))]

            def go(n):
                def worker(w):
                    torch.cuda.set_device(torch.device(dev))
                    with torch.cuda.stream(strs[w]):
                        for i in range(w, n, 2):
                            runs[w]([clouds[(i * B + j) % POOL] for j in range(B)])
                        strs[w].synchronize()
                ts = [threading.Thread(target=worker, args=(w,)) for w in range(2)]
                [t.start() for t in ts]
                [t.join() for t in ts]
            go(2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            go(8)
            torch.cuda.synchronize()
            sec2 = (time.perf_counter() - t0) / 8
            out["module_api"]["two_batches_in_flight"] = {"value": B / sec2, "ms_per_step_amortised": 1e3 * sec2, "steps": 8,
                                                          "ratio_to_engine": B / sec2 / value}
        except Exception as e:
            out["module_api"]["two_batches_in_flight"] = {"error": repr(e)[:300]}
    # (LAST of the extras: its copy streams are new HIP streams, and HIP deals streams to its few hardware queues in creation order -- created
    # earlier they moved the side streams of the extras after them onto the queues of their main streams: one frame 2.7 -> 3.1 ms, four
    # frames 837 -> 763 frames/s inside this process, unchanged as their own processes)
    # the boundary handing over HOST buffers: same step, same two streams, the clouds start in pinned host memory and their H2D
    # copies (3.2 MB per frame) are inside the timed region. Never the headline value (inputs resident in HBM is the contract).
    host = [c.cpu().pin_memory() for c in clouds]
    v, sec = engine_rate(cfg, B, 8, 2, n_streams=max(1, args.streams), host=host)
    out["value_host_input"] = {"value": v, "unit": "frames/s", "ms_per_step": 1e3 * sec, "steps": 8, "ratio_to_value": v / value,
                               "h2d_MB_per_step": sum(int(c.numel()) * 4 for c in host[:B]) / 1e6 if B <= POOL else None,
                               "note": "PCIe-inclusive: clouds in pinned host memory, H2D inside the timed region (%d stream(s)), double-buffered: a worker's next batch is copied on its own copy stream while the current one computes" % max(1, args.streams)}
    del host
    return out


def c5_stress_extra(dev, frames=16, iters=5):
    """BASELINE config 5 on the driver's clock: the dense-object stress -- Waymo-shape clouds at 0.05 m voxels
    (voxel (0.05, 0.05, 0.1) -> sparse grid [61, 3008, 3008]; 160k points -> ~126k active sites, 1M points -> ~0.9M) -- BATCHED over
    `frames` frames so that it is a bandwidth run, not a latency run: batched voxelizer + in-place level-0 index (canonical rows),
    sub-manifold rulebook, SubM 3x3x3 layers at 16 / 32 / 64 channels (gather-scatter). Per stage: HIP-event time of the call,
    ALGORITHMIC bytes (voxelize 4 N C + 4 M (C + 5); rulebook 16 N_in + 4 * 27 N_out; conv 4 (N_in C_in + N_out C_out)
    + 4 * 27 C_in C_out + 4 * 27 N_out table) -> TB/s and the fraction of the 8 TB/s HBM3E peak."""
    from cpd_amd.synthetic import WAYMO
    vs, shape = [0.05, 0.05, 0.1], [61, 3008, 3008]
    out = {"voxel_size": vs, "sparse_shape": shape, "frames_per_call": frames,
           "note": "algorithmic bytes / HIP-event time per call, %d frames per call, one stream; frac = of 8 TB/s" % frames}

    def timeit(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters * 1e-3

    def stage(sec, nbytes, flops=None):
        d = {"us_per_call": round(sec * 1e6, 1), "us_per_frame": round(sec * 1e6 / frames, 2), "algorithmic_MB": round(nbytes / 1e6, 1),
             "TBps": round(nbytes / sec / 1e12, 3), "frac_of_hbm_peak": round(nbytes / sec / 8.0e12, 4)}
        if flops is not None:
            d["useful_TFLOPs"] = round(flops / sec / 1e12, 1)
        return d

    for n_points, n_az, distinct in ((160000, 2650, frames), (1000000, 18000, min(frames, 4))):
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            host = list(ex.map(lambda s_: waymo_cloud(100 + s_, n_points=n_points, n_az=n_az), range(distinct)))
        pts = [torch.from_numpy(host[i % distinct]).to(dev) for i in range(frames)]
        del host
        vz = ops.Voxelizer(vs, WAYMO["point_cloud_range"], 5, 5, 1000000, device=torch.device(dev))
        if not vz.batch_supported(frames, 0):
            out["%dk_points" % (n_points // 1000)] = {"error": "batched voxelizer refuses this grid"}
            continue
        _, coords, _, feats, nvox, index = vz.batch(pts, index_z_extra=0, canonical=True)
        counts = nvox.tolist()
        m = counts[frames]
        coords = coords[:m]
        n_in = sum(int(p.shape[0]) for p in pts)
        rec = {"points_per_frame": n_points, "active_sites_per_frame": round(m / frames, 1)}
        t = timeit(lambda: vz.batch(pts, index_z_extra=0, canonical=True))
        rec["voxelize+mean_vfe+index"] = stage(t, 4.0 * n_in * 5 + 4.0 * m * 10)
        t = timeit(lambda: ops.rulebook_subm(coords, index))
        nbr = ops.rulebook_subm(coords, index)
        pairs = int((nbr >= 0).sum())
        rec["subm_pairs_per_site"] = round(pairs / max(m, 1), 2)
        rec["rulebook_subm"] = stage(t, 16.0 * m + 4.0 * 27 * m)
        for c in (16, 32, 64):
            x = torch.randn((m, c), device=dev)
            w = ops.pack_weight(torch.randn((27, c, c), device=dev) * 0.05)
            math = "f16x2" if c >= 32 else "f32"
            y = torch.empty((m, c), device=dev)
            t = timeit(lambda: ops.gather_conv(x, c, w, nbr, 27, m, c, out=y, math=math))
            rec["subm_conv_%d" % c] = dict(stage(t, 4.0 * (2 * m * c) + 4.0 * 27 * c * c + 4.0 * 27 * m, flops=2.0 * pairs * c * c), math=math)
            del x, y, w
        out["%dk_points" % (n_points // 1000)] = rec
        del pts, vz, coords, feats, index, nbr
        torch.cuda.empty_cache()
    return out


def train_step_extra(args, cfg, sd, dev, steps=12, warmup=4, clouds=None, frames=1):
    """Config 3 inside the default run: CenterPointTrainer.step on one frame per step (voxelize, training-mode forward, CenterHead
    targets + loss, backward, all-reduce no-op at N = 1, Adam, weight repack)."""
    from cpd_amd.synthetic import gt_boxes
    from cpd_amd.train_engine import CenterPointTrainer
    seeds = dist_utils.frame_seeds(0, POOL)
    clouds = [torch.from_numpy(c).cuda() for c in make_clouds(seeds, args.points)] if clouds is None else clouds
    gts = [torch.from_numpy(gt_boxes(s)).cuda() for s in seeds]
    tr = CenterPointTrainer(cfg, sd, device=dev, total_steps=steps + warmup, world_size=1)
    last = [None]

    def step(i):
        idx = [(i * frames + j) % POOL for j in range(frames)]
        last[0] = tr.step([clouds[k] for k in idx], torch.stack([gts[k] for k in idx]))

    sec = time_steps(step, steps, warmup)
    return {"ms_per_step": 1e3 * sec, "frames_per_s": frames / sec, "steps": steps, "frames_per_step": frames,
            "arithmetic": {"forward": tr.store.math, "gradients": tr.store.grad_math if tr.store.math != "f32" else "f32"},
            "batch_norm": "training mode (batch statistics)", "final_loss": float(last[0][0])}


def train_step_child(args, steps, warmup, frames):
    """`python bench.py --mode train` as a child process; its line cut down to the train_step record (None if it fails)."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--mode", "train", "--steps", str(steps), "--warmup", str(warmup), "--frames", str(frames),
           "--points", str(args.points), "--conv-math", args.conv_math, "--no-cpu-baseline", "--no-roofline"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
        d = json.loads(r.stdout.strip().splitlines()[-1])
        return {"ms_per_step": d["ms_per_step"], "frames_per_s": d["value"], "steps": steps, "warmup": warmup, "frames_per_step": frames,
                "arithmetic": d["config"].get("arithmetic"), "batch_norm": d["config"].get("batch_norm"), "final_loss": d["config"].get("final_loss"),
                "process": "child (python bench.py --mode train --frames %d; GPU_MAX_HW_QUEUES=%s)" % (frames, os.environ.get("GPU_MAX_HW_QUEUES", "8 by default in --mode train"))}
    except Exception as e:
        print("bench.py: train-step child failed (%r); measuring in-process" % (e,), file=sys.stderr)
        return None


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            names = [ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")]
        return "%s (%d hardware threads)" % (names[0], len(names)) if names else "unknown"
    except OSError:
        return "unknown"


def physical_cores():
    """distinct (physical id, core id) pairs of /proc/cpuinfo: the CORES of the box (SMT siblings counted once); None if unreadable"""
    try:
        seen, phys, core = set(), None, None
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("physical id"):
                    phys = ln.split(":", 1)[1].strip()
                elif ln.startswith("core id"):
                    core = ln.split(":", 1)[1].strip()
                elif not ln.strip():
                    if phys is not None and core is not None:
                        seen.add((phys, core))
                    phys = core = None
        if phys is not None and core is not None:
            seen.add((phys, core))
        return len(seen) or None
    except OSError:
        return None


def cpu_baseline(cfg, sd, clouds_np, full_frames=5, one_thread=True):
    """The oracle's un-fused restatement of the reference graph on the host CPU: `full_frames` full 160k-point frames on all
    hardware threads (value = 1 / median), then ONE frame on one thread (OpenMP team size set through libgomp; the voxelizer,
    rulebook builds and NMS scan are serial either way, as in the reference)."""
    import ctypes
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ref_pipeline
    from oracle import Oracle
    o = Oracle()
    threads = os.cpu_count() or 1
    if os.environ.get("OMP_NUM_THREADS", "").isdigit():      # `OMP_NUM_THREADS=k python bench.py` bounds the team
        threads = min(threads, max(1, int(os.environ["OMP_NUM_THREADS"])))
    phys = physical_cores()
    cores = min(threads, phys) if phys else threads          # `cores` = physical cores the team can occupy; `threads` = the OpenMP team
    # one untimed voxelizer call so that, as in the reference's generator object, the dense lookup
    # volume already exists (it is allocated once per worker, data_processor.py:133-144)
    o.voxelize(clouds_np[0][:1000], cfg.voxel_size, cfg.point_cloud_range, cfg.max_points_per_voxel, cfg.max_voxels)
    times = []
    for i in range(max(1, full_frames)):
        t0 = time.perf_counter()
        ref_pipeline.forward(o, cfg, sd, [clouds_np[i % len(clouds_np)]])
        times.append(time.perf_counter() - t0)
    med = sorted(times)[len(times) // 2]
    out = {"value": 1.0 / med, "unit": "frames/s", "cores": cores, "threads": threads, "cpu": cpu_model(), "kind": "port",
           "sample": "%d full 160k-point frames through the whole path (oracle/cpd_oracle.c, OpenMP team of %d threads on %d physical cores): "
                     "%s s, median %.1f s" % (len(times), threads, cores, "/".join("%.1f" % t for t in times), med)}
    if one_thread and threads > 1:
        try:
            gomp = ctypes.CDLL("libgomp.so.1")
            gomp.omp_set_num_threads(1)
            t0 = time.perf_counter()
            ref_pipeline.forward(o, cfg, sd, [clouds_np[0]])
            dt1 = time.perf_counter() - t0
            gomp.omp_set_num_threads(threads)
            out["one_thread"] = {"value": 1.0 / dt1, "unit": "frames/s", "cores": 1, "sample": "1 full frame, %.1f s" % dt1}
        except OSError:
            out["one_thread"] = None
    return out


def train_main(args, cfg, sd, dev, rank, world, distributed):
    """Config 3: one train step = voxelize + forward (batch-stat BN) + CenterHead loss + backward +
    ONE all-reduce of the flat gradient buffer over RCCL + fused Adam + weight repack."""
    from cpd_amd.synthetic import gt_boxes
    from cpd_amd.train_engine import CenterPointTrainer
    B = args.frames
    total = args.steps + args.warmup
    seeds = dist_utils.frame_seeds(rank, POOL)[:max(1, min(POOL, (total + 16) * B))]      # no more clouds than the run will touch
    clouds = [torch.from_numpy(c).cuda() for c in make_clouds(seeds, args.points)]
    gts = [torch.from_numpy(gt_boxes(s)).cuda() for s in seeds]
    POOL_T = len(seeds)
    tr = CenterPointTrainer(cfg, sd, device=dev, total_steps=max(total, 2), world_size=world, sync_bn=args.sync_bn)
    prof = ConvProfiler() if not args.no_roofline else None

    def step(i):
        idx = [(i * B + j) % POOL_T for j in range(B)]
        return tr.step([clouds[k] for k in idx], torch.stack([gts[k] for k in idx]))

    for i in range(args.warmup):
        step(i)
    dist_utils.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss, parts = step(args.warmup + i)
    torch.cuda.synchronize()
    dist_utils.barrier()
    local_elapsed = time.perf_counter() - t0
    elapsed = dist_utils.max_over_ranks(local_elapsed, device="cuda" if distributed else "cpu")
    per_rank = dist_utils.gather_floats(local_elapsed, device="cuda" if distributed else "cpu")
    if args.dump_outputs and rank == 0:
        # what the last timed step returned (its loss terms) and what it updated (a fixed sample of the flat parameter buffer)
        flat = tr.store.flat
        sample = torch.from_numpy(np.sort(np.random.default_rng(0).choice(flat.numel(), min(flat.numel(), 1 << 20), replace=False)))
        dump_outputs(args.dump_outputs, {"loss": loss.reshape(1).cpu(), "hm_loss": parts["hm_loss"].reshape(1).cpu(),
                                         "loc_loss": parts["loc_loss"].reshape(1).cpu(),
                                         "params_sample": flat.detach().reshape(-1)[sample.to(flat.device)].cpu()})
    comm = None
    if distributed and args.full:
        # the step's one collective, timed: (a) in place, HIP events around it in three more steps (includes waiting for the slowest
        # rank's backward); (b) alone, ten back-to-back all-reduces of the same flat buffer (ring / direct bandwidth over xGMI)
        tr.allreduce_events = []
        for i in range(3):
            step(total + 10 + i)
        torch.cuda.synchronize()
        in_step = [e0.elapsed_time(e1) for e0, e1 in tr.allreduce_events]
        tr.allreduce_events = None
        buf = torch.zeros_like(tr.store.grad)
        for _ in range(2):
            torch.distributed.all_reduce(buf)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(10):
            torch.distributed.all_reduce(buf)
        torch.cuda.synchronize()
        alone = (time.perf_counter() - t1) / 10
        nbytes = buf.numel() * 4
        comm = {"allreduce_in_step_ms": in_step, "allreduce_alone_ms": 1e3 * alone, "bytes": nbytes,
                "bus_GBps": 2.0 * (world - 1) / world * nbytes / alone / 1e9,
                "note": "one all-reduce of the flat fp32 gradient buffer per step, after the whole backward (not overlapped)"}
    out = {
        "metric": "train frames/sec (fwd+bwd+Adam), 160k-pt Waymo cloud", "value": world * B * args.steps / elapsed,
        "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": "configs[2]: CPD VoxelResBackBone8x + BEV head train step on Waymo-shape %d-point clouds, "
                               "%d frame(s)/GPU, 30 synthetic GT boxes/frame" % (args.points, B),
                   "frames_per_step_per_gpu": B, "parallelism": "data-parallel x%d, one RCCL all-reduce of the flat "
                   "gradient buffer (%.1f MB fp32) per step" % (world, tr.store.grad.numel() * 4 / 1e6),
                   "optimizer": "Adam(betas=(0.9,0.99)) + decoupled wd 1e-5 + OneCycle lr 3e-3 + grad-norm clip 32",
                   "batch_norm": ("training mode: batch statistics all-reduced over the ranks (SyncBatchNorm, --sync-bn)" if args.sync_bn else "training mode: batch statistics + running-stat update, local to the rank (no SyncBN, as the reference default)"),
                   "arithmetic": {"forward": tr.store.math, "input_and_weight_gradients": tr.store.grad_math if tr.store.math != "f32" else "f32",
                                  "note": "f16x2 = fp32 operands as two fp16 terms, three MFMA products, fp32 accumulation (fp32-level "
                                          "result); gradient tensors are pre-scaled into fp16's range by a power of two taken from "
                                          "their max |value| (exact; DESIGN.md 5a). Layers below 32 channels: fp32 MFMA."},
                   "final_loss": float(loss)},
    }
    if world > 1:
        dd = "cuda" if distributed else "cpu"
        out["per_rank"] = {"elapsed_s": per_rank, "frames_per_s": [args.steps * B / t for t in per_rank]}
    if world > 1 and args.full:
        # data-parallel invariants, checked across ranks: disjoint frame shards, identical parameters after the last step
        out["per_rank"].update({"first_frame_seed": [int(v) for v in dist_utils.gather_floats(seeds[0], device=dd)],
                                "param_checksum": dist_utils.gather_floats(float(tr.store.flat.double().abs().sum()), device=dd),
                                "param_first_words": dist_utils.gather_floats(float(tr.store.flat[:4096].double().sum()), device=dd)})
        pc = out["per_rank"]["param_checksum"]
        out["per_rank"]["parameters_identical_across_ranks"] = all(v == pc[0] for v in pc)
        out["collective"] = comm
    if prof is not None:
        with prof:
            for i in range(2):
                step(total + i)
            agg, conv_ms = prof.summary()
            if args.layers and rank == 0:
                per = len(prof.records) // 2
                for kname, fl, e0, e1, shp in prof.records[-per:]:
                    ms = e0.elapsed_time(e1)
                    print("%-34s n_out %7d  %3d->%4d kv %2d  %8.1f us  useful %6.1f TF  density %.2f" %
                          (kname, shp[0], shp[1], shp[2], shp[3], ms * 1e3, fl / ms / 1e9,
                           fl / (2.0 * shp[0] * shp[3] * shp[1] * shp[2])), file=sys.stderr)
        flops = sum(v[0] for v in agg.values())
        out["conv_fwd_dgrad"] = {"ms_per_step": conv_ms / 2, "tflops": flops / (conv_ms * 1e-3) / 1e12,
                                 "note": "cpd_gather_conv launches only (forward + input gradients), HIP events"}
    if rank == 0:
        print(json.dumps(out))
    dist_utils.shutdown()


def launch_check(args):
    """--launch-check: the N > 1 plumbing alone, any backend (gloo on CPUs in the tests, RCCL on the GPUs): ranks, CPU pinning,
    rendezvous, barrier, max-over-ranks, the per-rank clocks of the bench line and the train step's bucketed gradient all-reduce on a
    buffer of the real size -- the first 8-GPU run should meet nothing here for the first time."""
    rank, world, local = dist_utils.env_rank()
    cpus = dist_utils.pin_rank()
    backend = os.environ.get("CPD_DIST_BACKEND", "nccl")
    distributed = dist_utils.init(backend)
    dev = "cuda" if (distributed and backend == "nccl") else "cpu"
    if dev == "cuda":
        torch.cuda.set_device(local % max(1, torch.cuda.device_count()))
    dist_utils.barrier()
    slowest = dist_utils.max_over_ranks(1.0 + rank, device=dev)
    seeds = dist_utils.frame_seeds(rank, POOL)
    # the bench line's per-rank fields: every rank's own clock, whole-job throughput over the slowest one
    t0 = time.perf_counter()
    dist_utils.barrier()
    local_elapsed = 1.0 + 0.25 * rank + (time.perf_counter() - t0) * 0.0
    per_rank = dist_utils.gather_floats(local_elapsed, device=dev)
    whole_job = dist_utils.aggregate_throughput(48.0, local_elapsed, device=dev)
    # config 3's collective: 7.8 M fp32 gradients (31 MB) in two buckets that may overlap, then the averaged result
    n = int(os.environ.get("CPD_LAUNCH_CHECK_GRAD_FLOATS", str(7_800_000)))
    flat = torch.full((n,), float(rank + 1), dtype=torch.float32, device=dev)
    dist_utils.barrier()
    t0 = time.perf_counter()
    red = dist_utils.BucketedReduce(flat)
    red.start(n // 2, n)
    factor = red.finish()
    if dev == "cuda":
        torch.cuda.synchronize()
    ar_ms = 1e3 * (time.perf_counter() - t0)
    mean = float(flat[0]) * factor, float(flat[-1]) * factor
    ar_all = dist_utils.gather_floats(ar_ms, device=dev)
    aff = dist_utils.gather_ints([len(cpus), cpus[0] if cpus else -1, cpus[-1] if cpus else -1], device=dev)
    if rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": world, "gpus_arg": args.gpus, "max_over_ranks": slowest,
                          "rank0_frame_seeds": seeds, "backend": backend if distributed else None,
                          "per_rank": {"elapsed_s": per_rank, "allreduce_in_step_ms": ar_all,
                                       "cpu_affinity": [{"cpus": a[0], "first": a[1], "last": a[2]} for a in aff]},
                          "whole_job_units_per_s": whole_job, "allreduce_bytes": 4 * n, "allreduce_mean": mean,
                          "expected_mean": (world + 1) / 2.0}))
    dist_utils.shutdown()


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher around us: become the launcher (N ranks of this same command under torch.distributed.run)
        sys.exit(dist_utils.launch_ranks(args.gpus, os.path.abspath(__file__), sys.argv[1:]))
    rank, world, local = dist_utils.env_rank()
    if world != args.gpus and rank == 0:
        print("bench.py: --gpus %d but the launcher started %d rank(s); reporting n_gpus = %d" % (args.gpus, world, world),
              file=sys.stderr)
    if args.launch_check:
        return launch_check(args)
    if world > 1:
        dist_utils.pin_rank(local, int(os.environ.get("LOCAL_WORLD_SIZE", world)))      # a CPU slice per rank, NUMA order (dist_utils.rank_cpus)
    local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    # "nccl" is RCCL on ROCm; CPD_DIST_BACKEND=gloo lets several ranks share one GPU for functional tests
    distributed = dist_utils.init(os.environ.get("CPD_DIST_BACKEND", "nccl"), torch.device("cuda", local))

    cfg = ModelConfig(conv_math=args.conv_math, row_order=args.row_order, row_order_chunk=args.row_order_chunk, plan_rulebooks=bool(args.plan), plan_tile_rows=args.plan_tile, row_order_level0=bool(args.order_level0), pair_rows=bool(args.pair_rows),
                      pair_rows_level1=args.pair_rows == 2, pair_rows_dense=bool(args.dense_pairs), persistent_dense_map=bool(args.dense_map),
                      index_side_stream=bool(args.index_stream), deblock_side_stream=bool(args.deblock_stream),
                      batched_voxelizer_min_frames=args.vox_batch_min)
    sd = init_state_dict(cfg, seed=0)                 # same random-init weights on every rank
    dev = "cuda:%d" % local
    if args.mode == "train":
        return train_main(args, cfg, sd, dev, rank, world, distributed)
    S = max(1, args.streams)
    if args.api == "modules":
        S = 1
    engines = [CenterPointEngine(cfg, sd, device=dev, host_results=not args.device_results) for _ in range(S)] if args.api == "engine" else []
    streams = [torch.cuda.Stream(device=dev) for _ in range(S)]
    clouds_np = make_clouds(dist_utils.frame_seeds(rank, POOL), args.points)
    clouds = [torch.from_numpy(c).cuda() for c in clouds_np]
    B = args.frames
    torch.cuda.synchronize()

    host_clouds = [torch.from_numpy(c).pin_memory() for c in clouds_np] if args.host_input else None

    module_run = None

    def step(i, w=0):
        if module_run is not None:
            return module_run([clouds[(i * B + j) % POOL] for j in range(B)])
        if host_clouds is not None:      # boundary hands over host buffers: H2D inside the step
            return engines[w].forward([host_clouds[(i * B + j) % POOL].cuda(non_blocking=True) for j in range(B)])
        return engines[w].forward([clouds[(i * B + j) % POOL] for j in range(B)])

    def run_steps(n, S=S, keep=None):
        """n steps, dealt round-robin to S worker threads; each worker owns a HIP stream, an engine
        workspace and its frames' host-side count reads, so latency-bound phases of one frame
        (voxelizer, rulebooks, decode, NMS, count syncs) overlap the MFMA phases of the others.
        `keep`: dict step index -> that step's results (references only; digested after the timed region)."""
        if S == 1:
            for i in range(n):
                r = step(i)
                if keep is not None:
                    keep[i] = r
            return
        import threading

        def worker(w):
            torch.cuda.set_device(local)
            with torch.cuda.stream(streams[w]):
                for i in range(w, n, S):
                    r = step(i, w)
                    if keep is not None:
                        keep[i] = r
                streams[w].synchronize()

        ts = [threading.Thread(target=worker, args=(w,)) for w in range(S)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()

    barrier = dist_utils.barrier
    if args.api == "modules":
        module_run = module_api_runner(cfg, sd, dev, clouds, cfg.conv_math)

    run_steps(args.warmup)
    barrier()
    torch.cuda.synchronize()
    timed_results = {}
    t0 = time.perf_counter()
    run_steps(args.steps, keep=timed_results)
    torch.cuda.synchronize()
    barrier()
    local_elapsed = time.perf_counter() - t0
    elapsed = dist_utils.max_over_ranks(local_elapsed, device="cuda" if distributed else "cpu")
    per_rank = dist_utils.gather_floats(local_elapsed, device="cuda" if distributed else "cpu")
    # what the timed steps returned, digested AFTER the clock stopped: per-frame box counts + a hash over every kept box / score /
    # label of every frame (cpd_amd/digest.py). Step i of any run of this configuration sees the same frames, so the single-stream
    # pass below must reproduce these digests bit for bit -- the check that two batches in flight on two HIP streams computed what
    # one stream computes.
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, detection_arrays(timed_results[max(timed_results)]))
    from cpd_amd.digest import step_digest
    timed_digests = {i: step_digest(r) for i, r in sorted(timed_results.items())} if args.full else {}
    timed_results.clear()

    out = {
        "metric": "frames/sec voxelize->sparse3D->BEV->NMS, 160k-pt Waymo cloud",
        "value": world * args.steps * B / elapsed, "unit": "frames/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None,
        "dtype": {"f16x2": "f32 (split-fp16 x2 on the fp16 MFMA pipe: 3 products, fp32 accumulate)",
                  "bf16x3": "f32 (split-bf16 x3 on the bf16 MFMA pipe: 6 products, fp32 accumulate)", "f32": "f32"}[cfg.conv_math],
        "data": "synthetic" + (" (inputs in pinned host memory, H2D timed)" if args.host_input else ""),
        "results": "left on the device" if args.device_results else "copied to host memory inside the timed region",
        "api": "fused engine (cpd_amd.engine.CenterPointEngine)" if args.api == "engine" else
               "drop-in modules (cpd_amd.models.CenterPoint through batch_dict, eval-mode fusion)",
        "config": {"workload": "configs[1]: Waymo-shape %d-point cloud, CPD VoxelResBackBone8x + HeightCompression + "
                               "BaseBEVBackbone + CenterHead + rotated NMS, forward-only" % args.points,
                   "frames_per_step_per_gpu": B, "streams_per_gpu": S, "voxel_size": cfg.voxel_size, "sparse_shape": cfg.sparse_shape,
                   "parallelism": "frame-sharded replicas x%d, no data-path collective" % world,
                   "weights": "random-init (seed 0), eval-mode BN folded",
                   "sparse_row_order": {"taps": "strided levels in tap-pattern order (chunks of %d canonical rows sorted by neighbour pattern)" % cfg.row_order_chunk,
                                        "bricks": "strided levels in %d x %d (y, x) brick order per z-plane, 128-row tiles sorted by neighbour pattern; their "
                                                  "sub-manifold rulebooks carry a row plan (staged row-wave kernel)" % tuple(cfg.row_order_brick),
                                        "canonical": "canonical (b, z, y, x)"}[cfg.row_order],
                   "conv_math": {"bf16x3": "layers with >= 32 input channels: split-bf16 x3 (fp32 operands split exactly into 3 bf16 terms, "
                                           "6 bf16 MFMA products per fp32 multiply-add, fp32-level error); 5/16-channel sparse layers: fp32 MFMA",
                                 "f16x2": "layers with >= 32 input channels: split-fp16 x2 (fp32 operands written as 2 fp16 terms, 3 fp16 MFMA "
                                          "products per fp32 multiply-add, fp32 accumulation, fp32-level error); the 5-channel input layer: fp32 "
                                          "MFMA; the 16-channel level-1 layers: " +
                                          ("the same split-fp16 arithmetic on the K = 16 MFMA (v_mfma_f32_16x16x16_f16, gather_conv_h16_kernel), "
                                           "reading fp16-pair rows" if (cfg.pair_rows and cfg.pair_rows_level1) else "fp32 MFMA"),
                                 "f32": "fp32 MFMA everywhere"}[cfg.conv_math],
                   "pair_rows_dense": bool(cfg.pair_rows and cfg.pair_rows_dense) and cfg.conv_math == "f16x2",
                   "pair_rows": bool(cfg.pair_rows) and cfg.conv_math == "f16x2", "pair_rows_level1": bool(cfg.pair_rows and cfg.pair_rows_level1) and cfg.conv_math == "f16x2",
                   "activation_storage": ("between the sparse layers of levels %s: fp16-pair rows (each fp32 activation stored as its two fp16 "
                                          "terms h + l, 4 bytes per channel, split made once by the producing epilogue)%s; exported levels: fp32"
                                          % ("1-4" if cfg.pair_rows_level1 else "2-4",
                                             " -- and (batches of >= 8 frames) the stride-8 output, the densified BEV map and every dense map up to the "
                                             "head's hidden layer as pair maps as well (window_conv_f16p / tile_conv_f16p kernels); head output maps fp32"
                                             if cfg.pair_rows_dense else "; the BEV map and every dense activation: fp32"))
                   if (cfg.pair_rows and cfg.conv_math == "f16x2") else "fp32 everywhere",
                   "distinct_clouds_per_rank": POOL,
                   "range_guard": ("f16x2 range guard on: every conv epilogue records max |out|, the verdict rides with the step's count "
                                   "read-back, a step with an activation >= 2^15 is re-run with power-of-two pre-scaling (exact); re-runs "
                                   "in this run: %d" % sum(getattr(e, "range_reruns", 0) for e in engines))
                   if cfg.conv_math == "f16x2" and cfg.range_guard and engines else "n/a"},
    }

    single_results = {}
    if not args.no_roofline and args.api == "engine":
        # Second pass, same configuration (same streams / batch), with every cpd_gather_conv launch
        # bracketed by HIP events on its own launch stream.
        n_prof = min(args.steps, 6)
        # (the engines' side streams -- index chain, small-batch deblock -- are switched off for this pass and the next: a launch that
        # shares the chip with another stream's kernels is not a per-launch figure. Same kernels, same results either way.)
        side_was = (cfg.index_side_stream, cfg.deblock_side_stream)
        cfg.index_side_stream = cfg.deblock_side_stream = False
        with ConvProfiler() as prof, ClockSampler() as clk:
            run_steps(min(POOL // max(1, B) + 1, 4), 1)   # settle the allocator with the profiler's own temporaries in play
            torch.cuda.synchronize()
            prof.records.clear()
            prof.bytes_total = 0.0
            run_steps(n_prof, 1, keep=single_results)     # ONE stream: every launch owns the chip while it is timed
            agg, conv_ms = prof.summary()
            if args.layers and rank == 0:
                per = len(prof.records) // n_prof
                for kname, flops, e0, e1, shp in prof.records[-per:]:
                    ms = e0.elapsed_time(e1)
                    dense_fl = 2.0 * shp[0] * shp[3] * shp[1] * shp[2]
                    print("%-34s n_out %7d  %3d->%4d kv %2d  %8.1f us  useful %6.1f TF  density %.2f" %
                          (kname, shp[0], shp[1], shp[2], shp[3], ms * 1e3, flops / ms / 1e9, flops / dense_fl), file=sys.stderr)
        key, (flops, ms, launches) = max(agg.items(), key=lambda kv: kv[1][1])
        achieved = flops / (ms * 1e-3) / 1e12
        conv_flops = sum(v[0] for v in agg.values()) / (n_prof * B)        # algorithmic conv flop per frame
        conv_bytes = prof.bytes_total / (n_prof * B)                       # algorithmic conv HBM bytes per frame
        peak, peak_basis = kernel_peak(key)
        try:
            probe = mfma_power_probe(dev) if rank == 0 else None
        except Exception as e:                            # (a diagnostic must not take the line down)
            probe = {"error": repr(e)[:200]}
        out["roofline"] = {
            "bound": "mfma", "kernel": key, "achieved": achieved, "peak": peak, "unit": "TFLOP/s",
            "frac": achieved / peak, "peak_basis": peak_basis, "achieved_over_fp32_mfma_peak": achieved / PEAK_FP32_MFMA_TFLOPS,
            "clock_state": clk.summary(),
            "power_cap_note": "peak is the nominal 2.4 GHz figure; measured on this part (tools/mfma_power_probe.hip, tools/power_probe.py): a "
                              "loop of nothing but f16 MFMAs on register operands sustains 0.65 (random data) to 0.74 (half zeros) of it under "
                              "the 1400 W socket cap, and this kernel runs at 1.9-2.1 GHz for the same reason (DESIGN.md 4.1)",
            # the ceiling the cap leaves (VERDICT r5 #3a): the same MFMA instruction alone, timed in this process on this box -- `frac`
            # prices the kernel against the nominal 2.4 GHz peak, frac_of_power_capped against what the matrix pipe sustains under 1400 W
            "power_probe": probe,
            "power_capped_peak": (probe["relu_like_x_random"]["f16_mfma_tflops"] * peak / PEAK_BF16_MFMA_TFLOPS
                                  if probe and "relu_like_x_random" in probe and peak != PEAK_FP32_MFMA_TFLOPS else None),
            "power_capped_peak_basis": "cpd_mfma_burn (csrc/diag.hip): v_mfma_f32_16x16x32_f16 on register operands, nothing else in the loop, "
                                       "A = post-ReLU-like fp16 values (half zeros), B = random fp16 values, ~1.2 s sustained on this box right "
                                       "after the roofline pass; / the kernel's partial products per multiply-add",
            "traffic": pmc_traffic(key),
            "traffic_source": pmc_stamp(),
            "traffic_unit": "HBM-side bytes per launch (2*FETCH_SIZE + WRITE_SIZE from the committed rocprofv3 --pmc passes of this "
                            "command, %s; bench.py cannot collect counters itself)" % (os.path.relpath(pmc_summary_file() or "none", REPO)),
            "launches_per_frame": launches / (n_prof * B), "avg_launch_us": 1e3 * ms / launches,
            "algorithmic_gflop_per_launch": flops / launches / 1e9,
            "note": "per-launch figures from a single-stream pass (each launch owns the chip); the timed region ran %d batch(es) in "
                    "flight, so chip-level MFMA use over the step is chip_conv_tflops" % S,
            "chip_conv_tflops": conv_flops * out["value"] / world / 1e12,
            "chip_conv_over_fp32_mfma_peak": conv_flops * out["value"] / world / 1e12 / PEAK_FP32_MFMA_TFLOPS,
            "algorithmic_conv_gflop_per_frame": conv_flops / 1e9,
            "all_conv_kernels": {k: {"tflops": v[0] / (v[1] * 1e-3) / 1e12, "ms_per_frame": v[1] / (n_prof * B),
                                     "launches_per_frame": v[2] / (n_prof * B),
                                     "frac_of_its_peak": v[0] / (v[1] * 1e-3) / 1e12 / kernel_peak(k)[0]}
                                 for k, v in sorted(agg.items())},
        }

    if out.get("roofline") and out["roofline"].get("power_capped_peak"):
        out["roofline"]["frac_of_power_capped"] = out["roofline"]["achieved"] / out["roofline"]["power_capped_peak"]
    if not args.no_roofline and args.api == "engine":
        with HbmStageProfiler() as hp:
            run_steps(2, 1)
            out["hbm_stages"] = hp.summary(2 * B)
        # the whole path against the HBM roofline (north_star): all algorithmic bytes of a frame -- voxelizer, rulebooks, every
        # conv layer (sparse and dense), densify -- over the measured time per frame and the 8 TB/s peak. The path is bound by
        # the matrix pipe in its dense half, so this fraction is small by construction; the conv kernels' own ceiling is `frac`.
        stage_bytes = sum(v["algorithmic_MB_per_frame"] * 1e6 for k, v in out["hbm_stages"].items() if k != "sparse_conv_c<=16")
        path_bytes = conv_bytes + stage_bytes
        sec_per_frame = 1.0 / (out["value"] / world)
        cfg.index_side_stream, cfg.deblock_side_stream = side_was
        out["roofline"]["path_hbm_frac"] = path_bytes / sec_per_frame / 8.0e12
        out["roofline"]["path_algorithmic_MB_per_frame"] = path_bytes / 1e6
        out["roofline"]["path_hbm_floor_ms_per_frame"] = path_bytes / 8.0e12 * 1e3
        out["hbm_stages"]["note"] = ("algorithmic bytes (SURVEY 8d) / HIP-event time of each call (one call = all its launches), "
                                     "single stream; peak = 8 TB/s nominal HBM3E")

    if args.full:
        # results_digest: the timed steps (S batches in flight) against the same steps on ONE stream
        if not single_results and not args.no_digest_check:
            run_steps(min(2, args.steps), 1, keep=single_results)
            torch.cuda.synchronize()
        single_digests = {i: step_digest(r) for i, r in sorted(single_results.items())}
        single_results.clear()
        common = sorted(set(single_digests) & set(timed_digests))
        mismatch = [i for i in common if single_digests[i] != timed_digests[i]]
        d0 = timed_digests[min(timed_digests)] if timed_digests else ([], [], None)
        out["results_digest"] = {
            "timed_steps": [timed_digests[i][2] for i in sorted(timed_digests)],
            "boxes_per_frame_step0": d0[0], "boxes_step0": sum(d0[0]),
            "single_stream_steps": [single_digests[i][2] for i in sorted(single_digests)],
            "steps_compared": len(common), "equal_to_single_stream_pass": (not mismatch) if common else None,
            "all_timed_steps_equal": (len({timed_digests[i][2] for i in timed_digests}) == 1) if (timed_digests and POOL % B == 0 and B == POOL) else None,
            "note": "per step: BLAKE2 over every frame's kept boxes / scores / labels (cpd_amd/digest.py). The timed region ran %d batch(es) "
                    "in flight on %d HIP stream(s) / worker thread(s); the single-stream pass re-ran the same steps on one stream after "
                    "the clock stopped. Equal digests = bit-identical detections." % (S, S)}
        if mismatch and not args.no_digest_check:
            print(json.dumps(out["results_digest"]), file=sys.stderr)
            raise SystemExit("bench.py: results of timed step(s) %s differ from the single-stream pass (results_digest)" % mismatch)
    if world > 1:
        out["per_rank"] = {"elapsed_s": per_rank, "frames_per_s": [args.steps * B / t for t in per_rank],
                           "note": "each rank's own clock around its %d timed steps (value uses the slowest)" % args.steps}

    if world == 1 and not args.no_extras and args.api == "engine" and not args.host_input:
        engines.clear()
        torch.cuda.empty_cache()
        out.update(extras(args, cfg, sd, dev, clouds, out["value"], streams))
        torch.cuda.empty_cache()
        # config 3 is a training JOB: measured as one -- its own process (python bench.py --mode train ...: own HIP context, no streams and
        # engines left over from the inference runs above, GPU_MAX_HW_QUEUES as a training process sets it) -- while this process
        # idles; in-process (round 4's form, a dozen steps among the inference extras' leftovers) if the child fails
        out["train_step"] = train_step_child(args, 40, 10, 1) or train_step_extra(args, cfg, sd, dev, clouds=clouds)
        torch.cuda.empty_cache()
        # config 3 prescribes one frame per GPU; one frame does not fill the chip -- the same step at 8 frames per GPU for comparison
        out["train_step_8frames"] = (train_step_child(args, 10, 3, 8) or
                                     train_step_extra(args, cfg, sd, dev, steps=6, warmup=2, clouds=clouds, frames=8))
        torch.cuda.empty_cache()
        try:
            out["c5_stress"] = c5_stress_extra(dev)
        except Exception as e:                              # an extra must not take the headline line down
            out["c5_stress"] = {"error": repr(e)[:300]}

    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(cfg, sd, clouds_np)

    if rank == 0:
        print(json.dumps(out))
    dist_utils.shutdown()


if __name__ == "__main__":
    main()
