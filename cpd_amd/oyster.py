"""GPU drop-in for CPD's OYSTER pseudo-label generator (cpd/unsupervised_core/oyster.py, with outline_utils.py corner_align,
drop_cls and TrackSmooth): <seq>/<seq>_outline_MFCF.pkl (or <seq>/<seq>.pkl and the NNNN.npy frames) go in,
<seq>/<seq>_outline_OYSTER.pkl comes out. Frames without boxes go through ground removal, DBSCAN and box_fit as HIP kernels
(csrc/outline.hip) in chunks; the tracker over the per-frame boxes is cpd_amd.tracker on the host; the size consensus of every
track and the corner alignment of its boxes are one launch of csrc/oyster.hip (cpd_oyster_align_tracks).

Exactness contract: ids, classes and dif are the host's own; l, w, h, yaw and z of the aligned boxes are the
restatement's bit for bit, x and y agree to one float32 ulp of cos / sin times the offset (device libm against the host's before
the float32 rounding), 1e-6. Per-frame boxes: §5l.
"""
import os
import pickle as pkl
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import outline
from .outline import DBSCAN_GENERATOR_CONFIG, _get, _paths, drop_cls
from .seq_io import dispatch_outline_box, dtype_runs, frame_path, gpu_modules, prefetched_chunks, run_sequences
from .tracker import TrackSmooth

# GeneratorConfig of tools/cfgs/dataset_configs/waymo_unsupervised/waymo_unsupervised_oyster.yaml: the OutlineFitter arguments and
# the tracker block, with the size / yaw windows on and short tracks removed
OYSTER_GENERATOR_CONFIG = dict(
    DBSCAN_GENERATOR_CONFIG,
    state_func_covariance=10, measure_func_covariance=0.1, prediction_score_decay=0.025, LiDAR_scanning_frequency=10,
    max_prediction_num=16, max_prediction_num_for_new_object=3, lwh_win_size=20, yaw_win_size=10,
    input_score=-0.5, init_score=-0.5, update_score=-0.5, post_score=1.4, latency=-1, remove_short_track=10)
OYSTER_CONFIG = dict(InitLabelGenerator='OYSTER', GeneratorConfig=OYSTER_GENERATOR_CONFIG)

MIN_TRACK_LEN = 6      # oyster.py:93, 123: shorter tracks are neither aligned nor written
TOP_FRACTION = 0.95    # oyster.py:106


def track_top(n):
    """oyster.py:106-108: the number of nearest boxes whose size is averaged, as Python evaluates it (1 - 0.95 is
    0.050000000000000044: 3 up to n = 79, 4 from n = 80, 5 from n = 100)."""
    return max(3, int(n * (1 - TOP_FRACTION)))


def launch_align(d_boxes, d_off, d_top, d_out):
    """cpd_oyster_align_tracks on device tensors, on the current stream: d_boxes / d_out [N, 7] float64, d_off [T + 1] and d_top
    [T] int32. Nothing is checked or read back here."""
    _, _lib = gpu_modules()
    _lib.check(_lib.lib().cpd_oyster_align_tracks(_lib.ptr(d_boxes), _lib.ptr(d_off), _lib.ptr(d_top), int(d_top.shape[0]),
                                                  int(d_boxes.shape[0]), _lib.ptr(d_out), _lib.stream()),
               "cpd_oyster_align_tracks")
    return d_out


def align_tracks(boxes, track_off, device=None):
    """oyster.py:89-115 with corner_align for every track in one launch. boxes [N, 7] float64 in track-major order (each
    track's rows in frame order), track_off [T + 1] their offsets; returns the aligned boxes [N, 7] float64. The offsets are
    checked here, on the host, before they travel."""
    torch, _lib = gpu_modules()
    boxes = np.ascontiguousarray(boxes, np.float64).reshape(-1, 7)
    off = np.asarray(track_off)
    if off.ndim != 1 or len(off) < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError("cpd_amd.oyster: track_off must be a vector of T + 1 integers")
    n, t = len(boxes), len(off) - 1
    if off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
        raise _lib.CpdHipError("cpd_oyster_align_tracks failed: CPD_ERR_ARG (track_off must rise from 0 to the %d rows)" % n)
    if t == 0 or n == 0:
        return np.empty_like(boxes)
    dev = torch.device(device if device is not None else "cuda")
    top = np.array([track_top(int(k)) for k in np.diff(off)], np.int32)
    with torch.cuda.device(dev):
        d_out = launch_align(torch.from_numpy(boxes).to(dev), torch.from_numpy(off.astype(np.int32)).to(dev),
                             torch.from_numpy(top).to(dev), torch.empty((n, 7), dtype=torch.float64, device=dev))
        return d_out.cpu().numpy()


def collect_tracks(tracker, n_frames):
    """oyster.py:70-86: {id: {frame: [box, cls, dif]}} in first-seen order, from the frames that keep more than one object
    once Dis_Small and Dis_Large are dropped."""
    tracks = {}
    for i in range(n_frames):
        objs, ids, cls, dif = tracker.get_current_frame_objects_and_cls(i)
        objs, cls, ids, dif, _, _ = drop_cls(objs, cls, dif=dif, ids=ids)
        if len(ids) <= 1:
            continue
        for j, ob_id in enumerate(ids):
            tracks.setdefault(ob_id, {})[i] = [objs[j], cls[j], dif[j]]
    return tracks


def write_frames(infos, tracks):
    """oyster.py:117-148: the kept tracks regrouped by frame, tracks in first-seen order, into infos."""
    rows = {}
    for ob_id, track in tracks.items():
        if len(track) < MIN_TRACK_LEN:
            continue
        for frame, (box, cls, dif) in track.items():
            r = rows.setdefault(frame, ([], [], [], []))
            r[0].append(box), r[1].append(ob_id), r[2].append(cls), r[3].append(dif)
    for i, info in enumerate(infos):
        if i in rows:
            box, ids, cls, dif = (np.array(v) for v in rows[i])
        else:
            box, ids, cls, dif = np.empty(shape=(0, 7)), np.empty(shape=(0,)), np.empty(shape=(0,)), np.empty(shape=(0,))
        info['outline_box'], info['outline_ids'], info['outline_cls'], info['outline_dif'] = box, ids, cls, dif
    return infos


class OYSTER:
    """oyster.py OYSTER: the same file contract. Behaviours of the reference kept on purpose:
      * the input is <seq>_outline_MFCF.pkl where it exists, else <seq>.pkl; a frame whose info carries 'outline_box' brings
        its detections, any other frame's NNNN.npy[:, 0:3] goes through ground removal, DBSCAN and box_fit;
      * the tracker sees the RAW box_fit boxes: get_box_cls / drop_cls are not applied before it (outline.outline_frames does);
      * NO CACHE: the reference's "return the existing output" block is commented out, so the output is recomputed and
        overwritten on every call -- unlike cpd_amd.outline.DBSCAN and cpd_amd.mfcf.MFCF, which return an existing file;
      * after the tracker every frame drops Dis_Small / Dis_Large, and a frame left with one object or none contributes
        nothing: a frame's only object is lost too;
      * tracks are collected per id in first-seen order; a track with fewer than 6 entries is neither aligned nor written;
      * the size consensus is the mean l, w of the max(3, int(n * (1 - 0.95))) boxes nearest the sensor, and corner_align
        keeps the candidate centre FARTHEST from the origin (its arg_min is an argmax), the first on ties; z comes back
        rounded to float32 (the float32 pose matrix);
      * a frame's rows are ordered by the first appearance of their track, not by detection order;
      * frames without rows get np.empty((0, 7)) and three np.empty((0,)).
    Frames that need the per-frame chain run in chunks of `chunk` (OutlineGPU.frames_boxes), their reads a chunk ahead on a
    thread pool; a sequence whose pickle carries boxes for every frame launches none of it."""

    def __init__(self, seq_name, root_path, config, device=None, chunk=16):
        self.seq_name, self.root_path, self.dataset_cfg = seq_name, root_path, config
        self.device, self.chunk = device, int(chunk)
        self._gpu = None
        if self.chunk < 1:
            raise ValueError("cpd_amd.oyster: chunk must be at least 1")

    @property
    def gpu(self):
        if self._gpu is None:
            self._gpu = outline.OutlineGPU(outline._params(_get(self.dataset_cfg, "GeneratorConfig")), self.device)
        return self._gpu

    def per_frame_boxes(self, infos, pool=None):
        """oyster.py:48-64: every frame's detections (and the poses)."""
        seq_dir = os.path.join(self.root_path, self.seq_name)
        all_labels = [info['outline_box'] if 'outline_box' in info else None for info in infos]
        need = [(i, frame_path(seq_dir, i)) for i, b in enumerate(all_labels) if b is None]
        for idx, frames in prefetched_chunks(need, self.chunk, pool=pool):   # the next chunk's reads overlap this chunk's kernels
            for r0, r1 in dtype_runs(frames, self.chunk):                    # one dtype per launch sequence
                for i, boxes in zip(idx[r0:r1], self.gpu.frames_boxes(frames[r0:r1])):
                    all_labels[i] = boxes
        return all_labels, [info['pose'] for info in infos]

    def generate_outline_box(self, pool=None):
        method = _get(self.dataset_cfg, "InitLabelGenerator")
        in_pkl, out_pkl = _paths(self.seq_name, self.root_path, method)
        mfcf_pkl = _paths(self.seq_name, self.root_path, 'MFCF')[1]
        with open(mfcf_pkl if os.path.exists(mfcf_pkl) else in_pkl, 'rb') as f:
            infos = pkl.load(f)
        all_labels, all_pose = self.per_frame_boxes(infos, pool)
        tracker = TrackSmooth(_get(self.dataset_cfg, "GeneratorConfig"))
        tracker.tracking(all_labels, all_pose)
        tracks = collect_tracks(tracker, len(infos))
        kept = [t for t in tracks.values() if len(t) >= MIN_TRACK_LEN]
        if kept:
            off = np.zeros(len(kept) + 1, np.int64)
            off[1:] = np.cumsum([len(t) for t in kept])
            aligned = align_tracks(np.array([e[0] for t in kept for e in t.values()]), off, self.device)
            for t, o in zip(kept, off):
                for k, e in enumerate(t.values()):
                    e[0] = aligned[o + k]
        write_frames(infos, tracks)
        with open(out_pkl, 'wb') as f:
            pkl.dump(infos, f)
        return infos

    def __call__(self):
        return self.generate_outline_box()


def create_oyster(seq_names, root_path, dataset_cfg, device=None, chunk=16):
    """Single-process sequence driver in place of the dataset's multiprocessing.Pool(16) (forked workers must not each open the
    GPU): every sequence through one GPU context, the .npy reads on a small thread pool while the GPU works."""
    with ThreadPoolExecutor(4) as pool:
        return run_sequences(lambda s: OYSTER(s, root_path, dataset_cfg, device, chunk), seq_names,
                             lambda o: o.generate_outline_box(pool))


def compute_outline_box(seq_name, root_path, dataset_cfg):
    """cpd/unsupervised_core/__init__.py compute_outline_box: InitLabelGenerator 'DBSCAN' (outline.DBSCAN), 'OYSTER' and 'MFCF'
    (mfcf.MFCF), then LabelRefiner 'C_PROTO' (cproto_refine.C_PROTO). mfcf's and outline's own dispatchers keep their narrower
    contracts."""
    from .mfcf import MFCF
    return dispatch_outline_box(seq_name, root_path, dataset_cfg, {'DBSCAN': outline.DBSCAN, 'OYSTER': OYSTER, 'MFCF': MFCF},
                                ('C_PROTO',), "oyster")
