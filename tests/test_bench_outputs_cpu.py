"""`bench.py --dump-outputs DIR`: what the last timed step computed, as float32 .npy files within the size budget, on a
sample of the batch that is the same in every run (two builds are compared file by file)."""
import os

import numpy as np
import torch

import bench


def _stages(n, c=3, h=8, w=8):
    # stage k, image i holds the value 100 k + i everywhere: a dumped image names its source
    return [torch.full((n, c, h, w), 100.0 * k) + torch.arange(n, dtype=torch.float32).view(n, 1, 1, 1) for k in range(1, 6)]


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_default_geometry_fits_the_budget(tmp_path):
    st = _stages(64, h=256, w=256)
    names = ['nearest', 'bilateral', 'wbmanual', 'gamma', 'gtmmanual']
    bench.dump_outputs(str(tmp_path), st[-1], st, names)
    got = _read(str(tmp_path))
    assert sorted(got) == ['output', 'stage1_nearest', 'stage2_bilateral', 'stage3_wbmanual', 'stage4_gamma']
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= bench.DUMP_BYTES
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got['output'], st[-1].numpy())                      # the forward's return value, whole
    pick = bench.dump_sample(64, 4)
    assert len(set(pick.tolist())) == 4 and pick.tolist() == sorted(pick.tolist())
    for j, k in enumerate(sorted(got)[1:]):
        assert np.array_equal(got[k], st[j].numpy()[pick.numpy()]), k


def test_dump_outputs_samples_a_large_batch_the_same_way_every_run(tmp_path, monkeypatch):
    # arrays that fill the budget exactly (10 images of one stage) once every file's header allowance is set aside
    monkeypatch.setattr(bench, 'DUMP_BYTES', 5 * bench.NPY_HEADER_BYTES + 10 * 3 * 8 * 8 * 4)
    st = _stages(32)
    names = list('abcde')
    runs = []
    for r in range(2):
        d = str(tmp_path / str(r))
        bench.dump_outputs(d, st[-1], st, names)
        runs.append(_read(d))
        assert sum(a.nbytes for a in runs[-1].values()) == 10 * 3 * 8 * 8 * 4
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= bench.DUMP_BYTES
    assert sorted(runs[0]) == sorted(runs[1]) and all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0])
    out = runs[0]['output'][:, 0, 0, 0] - 500
    assert list(out) == bench.dump_sample(32, 6).tolist()                      # 10 - 4 earlier stages x 1 image
    assert runs[0]['stage1_a'][:, 0, 0, 0].tolist() == [100 + bench.dump_sample(32, 1).item()]
