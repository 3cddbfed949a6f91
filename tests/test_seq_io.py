"""cpd_amd.seq_io: the chunked reader, the dtype runs and the sliding-window cache of the pseudo-label drivers, on temporary
.npy files and without a GPU."""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from cpd_amd import seq_io as S


@pytest.fixture()
def seq_dir(tmp_path):
    """Seven frames NNNN.npy of [i + 1, 5] rows whose first column is the frame index."""
    for i in range(7):
        np.save(S.frame_path(str(tmp_path), i), np.full((i + 1, 5), float(i), np.float32))
    return str(tmp_path)


def test_frame_path_and_load_xyz(seq_dir):
    assert S.frame_path(seq_dir, 3) == os.path.join(seq_dir, "0003.npy")
    xyz = S.load_xyz(S.frame_path(seq_dir, 3))
    assert xyz.shape == (4, 3) and (xyz == 3.0).all()


@pytest.mark.parametrize("chunk", [1, 3, 7, 50])
def test_prefetched_chunks_yields_every_index_once_in_order(seq_dir, chunk):
    paths = [S.frame_path(seq_dir, i) for i in range(7)]
    got = list(S.prefetched_chunks(paths, chunk))
    assert [i for idx, _ in got for i in idx] == list(range(7))
    assert all(len(idx) == len(frames) <= chunk for idx, frames in got)
    assert len(got) == -(-7 // chunk)
    for idx, frames in got:
        for i, f in zip(idx, frames):
            assert f.shape == (i + 1, 3) and (f == float(i)).all()


def test_prefetched_chunks_of_nothing():
    assert list(S.prefetched_chunks([], 4)) == []


def test_prefetched_chunks_takes_index_path_pairs(seq_dir):
    need = [(i, S.frame_path(seq_dir, i)) for i in (1, 4, 5)]
    got = list(S.prefetched_chunks(need, 2))
    assert [idx for idx, _ in got] == [[1, 4], [5]]
    assert [[len(f) for f in frames] for _, frames in got] == [[2, 5], [6]]


def test_prefetched_chunks_reads_at_most_one_chunk_ahead():
    lock, calls = threading.Lock(), []

    def load(path):
        with lock:
            calls.append(path)
        return path

    chunk, n = 3, 14
    for k, (idx, frames) in enumerate(S.prefetched_chunks(list(range(n)), chunk, load=load)):
        assert frames == idx
        with lock:      # reads submitted so far: this chunk's and the next one's, never a third
            assert len(calls) <= min(n, (k + 2) * chunk)
            assert set(calls) <= set(range(min(n, (k + 2) * chunk)))
    assert sorted(calls) == list(range(n))


def test_prefetched_chunks_leaves_the_callers_pool_open(seq_dir):
    paths = [S.frame_path(seq_dir, i) for i in range(5)]
    with ThreadPoolExecutor(2) as pool:
        assert len(list(S.prefetched_chunks(paths, 2, pool=pool))) == 3
        assert pool.submit(lambda: 7).result() == 7      # a pool that was shut down refuses new work
        gen = S.prefetched_chunks(paths, 2, pool=pool)
        next(gen)
        gen.close()                                      # abandoned half way
        assert pool.submit(lambda: 8).result() == 8


def test_dtype_runs_split_at_dtype_changes_and_at_chunk():
    h, f = np.zeros((2, 3), np.float16), np.zeros((2, 3), np.float32)
    frames = [h] * 5 + [f] * 2 + [h] * 3
    assert S.dtype_runs(frames, 4) == [(0, 4), (4, 5), (5, 7), (7, 10)]
    assert S.dtype_runs(frames, 16) == [(0, 5), (5, 7), (7, 10)]
    assert S.dtype_runs(frames, 1) == [(i, i + 1) for i in range(10)]
    assert S.dtype_runs([], 4) == []


def _cache(seq_dir, pool, n=7):
    loads, uploads = [], []

    def load(j):
        loads.append(j)
        path = S.frame_path(seq_dir, j)
        return np.load(path) if os.path.exists(path) else None

    def upload(j, host):
        uploads.append(j)
        return ("dev", j, host.shape)

    return S.SweepCache(pool, n, load, upload), loads, uploads


def test_sweep_cache_loads_and_uploads_a_frame_once(seq_dir):
    with ThreadPoolExecutor(2) as pool:
        cache, loads, uploads = _cache(seq_dir, pool)
        for j in (-1, 7, 2, 2):     # outside 0..n-1: ignored; asked twice: read once
            cache.want(j)
        assert cache.get(2) == ("dev", 2, (3, 5))
        assert cache.get(2) is cache.get(2)
        cache.want(2)               # already uploaded: no second read
        assert cache.get(5) == ("dev", 5, (6, 5))    # get without want reads too
    assert sorted(loads) == [2, 5] and uploads == [2, 5]


def test_sweep_cache_gives_none_for_a_missing_file(seq_dir):
    os.remove(S.frame_path(seq_dir, 4))
    with ThreadPoolExecutor(2) as pool:
        cache, loads, uploads = _cache(seq_dir, pool)
        assert cache.get(4) is None and cache.get(4) is None
    assert loads == [4] and uploads == []


def test_sweep_cache_drop_before_forgets_uploads(seq_dir):
    with ThreadPoolExecutor(2) as pool:
        cache, loads, uploads = _cache(seq_dir, pool)
        for j in range(4):
            cache.get(j)
        cache.drop_before(2)
        assert sorted(cache.dev) == [2, 3]
        cache.get(3)
        assert uploads == [0, 1, 2, 3]
        cache.get(1)                # forgotten: read and uploaded again
    assert uploads == [0, 1, 2, 3, 1] and loads.count(1) == 2


def test_run_sequences_hands_the_gpu_object_on():
    class Stage:
        def __init__(self, name):
            self.name, self._gpu = name, None

    seen = []

    def run(o):
        seen.append(o._gpu)
        if o._gpu is None:
            o._gpu = "gpu of " + o.name
        return o.name.upper()

    assert S.run_sequences(Stage, ["a", "b", "c"], run) == ["A", "B", "C"]
    assert seen == [None, "gpu of a", "gpu of a"]
    assert S.run_sequences(Stage, [], run) == []
