"""What the pseudo-label generators and refiners (outline, ppscore, cproto, cproto_refine, mfcf, oyster) share on the host: the
lazy GPU imports, the frame files of a sequence, the chunked and the sliding-window readers that keep the .npy reads ahead of
the kernels, the split into runs of one dtype, and the sequence and method dispatch of the drivers. No module of the family is
imported here at load time, so any of them may import this one."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np


def gpu_modules():
    """(torch, _lib), imported on first use: the host-only halves of the generators work without either."""
    import torch
    from . import _lib
    return torch, _lib


def _get(cfg, name, default=None):
    if isinstance(cfg, dict):
        return cfg.get(name, default)
    return getattr(cfg, name, default)


def _has(cfg, name):
    return name in cfg if isinstance(cfg, dict) else hasattr(cfg, name)


def frame_path(seq_dir, i):
    return os.path.join(seq_dir, str(i).zfill(4) + '.npy')


def load_xyz(path):
    return np.load(path)[:, 0:3]


def prefetched_chunks(items, chunk, load=load_xyz, pool=None):
    """(indices, frames) per chunk of `chunk` items, in order. items: paths (their indices are their positions) or
    (index, path) pairs. The next chunk's reads run on the pool (the caller's, or a small one of its own) while the caller works
    on this chunk; no more than two chunks' reads are ever outstanding."""
    items = [it if isinstance(it, tuple) else (k, it) for k, it in enumerate(items)]
    chunks = [items[c:c + chunk] for c in range(0, len(items), chunk)]
    if not chunks:
        return
    own_pool = pool is None
    pool = ThreadPoolExecutor(4) if own_pool else pool
    read = lambda c: [pool.submit(load, path) for _, path in c]
    try:
        futs = read(chunks[0])
        for k, c in enumerate(chunks):
            frames = [f.result() for f in futs]
            futs = read(chunks[k + 1]) if k + 1 < len(chunks) else []
            yield [i for i, _ in c], frames
    finally:
        if own_pool:
            pool.shutdown()


def dtype_runs(frames, chunk):
    """Runs (c0, c1) of at most `chunk` consecutive frames of one dtype (the ground projection's arithmetic is per dtype)."""
    runs, c0 = [], 0
    while c0 < len(frames):
        c1 = c0 + 1
        while c1 < len(frames) and c1 - c0 < chunk and np.asarray(frames[c1]).dtype == np.asarray(frames[c0]).dtype:
            c1 += 1
        runs.append((c0, c1))
        c0 = c1
    return runs


class SweepCache:
    """The frames 0..n-1 of a sequence under a sliding window: frame j is read once (load(j) on the pool, from want(j) on),
    uploaded once (upload(j, host) at its first get) and forgotten by drop_before once no window reaches it. load returns None
    for a missing file, and so does get. want ignores a j outside 0..n-1; how far ahead to ask is the caller's policy."""

    def __init__(self, pool, n, load, upload):
        self.pool, self.n, self.load, self.upload = pool, n, load, upload
        self.reads, self.dev = {}, {}

    def want(self, j):
        if 0 <= j < self.n and j not in self.reads and j not in self.dev:
            self.reads[j] = self.pool.submit(self.load, j)

    def get(self, j):
        if j not in self.dev:
            self.want(j)
            host = self.reads.pop(j).result()
            self.dev[j] = None if host is None else self.upload(j, host)
        return self.dev[j]

    def drop_before(self, j):
        for k in [k for k in self.dev if k < j]:
            del self.dev[k]


def run_sequences(make, seq_names, run):
    """[run(make(s)) for s in seq_names] with the GPU object (its buffers, `_gpu`) handed from one sequence's object to the
    next: the single-process driver in place of the dataset's multiprocessing.Pool(16), whose forked workers must not each
    open the GPU."""
    out, gpu = [], None
    for s in seq_names:
        o = make(s)
        o._gpu = gpu
        out.append(run(o))
        gpu = o._gpu
    return out


def dispatch_outline_box(seq_name, root_path, dataset_cfg, generators, refiners, module):
    """cpd/unsupervised_core/__init__.py compute_outline_box: the InitLabelGenerator out of `generators` (name -> class), then
    the LabelRefiner where `refiners` names it ('C_PROTO' is the only one there is). Any other name is refused in `module`'s
    name: each module's compute_outline_box keeps its own contract."""
    suc = None
    if _has(dataset_cfg, 'InitLabelGenerator'):
        method = _get(dataset_cfg, 'InitLabelGenerator')
        if method not in generators:
            raise NotImplementedError("cpd_amd.%s: InitLabelGenerator %r has no GPU drop-in here (only %s)"
                                      % (module, method, ", ".join(repr(g) for g in generators)))
        suc = generators[method](seq_name, root_path, dataset_cfg)()
    if _has(dataset_cfg, 'LabelRefiner'):
        refiner = _get(dataset_cfg, 'LabelRefiner')
        if refiner not in refiners:
            raise NotImplementedError("cpd_amd.%s: LabelRefiner %r has no GPU drop-in here (only %s)"
                                      % (module, refiner, ", ".join(repr(r) for r in refiners) or "none"))
        from .cproto_refine import C_PROTO
        suc = C_PROTO(seq_name, root_path, dataset_cfg)()
    return suc
