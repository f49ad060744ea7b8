"""The grouping kernels beyond the 32-bit element range (include/tsdf_group.h: all global indexing is in 64 bits): one call
whose ``index`` output ends beyond element 2^31, and one whose cloud does.  The position at the far end is compared with
the same position in a small call, which is compared with the numpy restatement (tests/group_ref.py).  The positions that
need no check carry a non-zero input status and are not read."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_ref as gr  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _need_memory(dev):
    free, _ = torch.cuda.mem_get_info(dev)
    assert free > 10 * 2 ** 30, "this test needs 10 GiB of device memory"


def _same(a, b):
    return all(x is None and y is None or torch.equal(x.view(torch.int32) if x.dtype is torch.float32 else x,
                                                      y.view(torch.int32) if y.dtype is torch.float32 else y) for x, y in zip(a, b))


def test_an_index_output_that_ends_beyond_2_31_elements(pkg):
    dev = torch.device("cuda:0")
    _need_memory(dev)
    P, C, K = 4, 512, 128
    n = 2 ** 31 // (C * K) + 2                                # 32770 positions of 65536 elements
    assert (n - 1) * C * K >= 2 ** 31
    live = [0, n - 1]
    clouds = gr.random_clouds(2, P, seed=31)
    queries = gr.random_clouds(2, C, seed=32)
    want = gr.knn(clouds, K, queries)
    small = pkg.knn_groups(torch.from_numpy(clouds).to(dev), K, queries=torch.from_numpy(queries).to(dev), dist2=False)
    assert gr.same_knn(type(small)(*[None if t is None else t.cpu().numpy() for t in small]), want) is None
    cloud = torch.zeros((n, P, 3), device=dev)
    query = torch.zeros((n, C, 3), device=dev)
    cloud[live], query[live] = torch.from_numpy(clouds).to(dev), torch.from_numpy(queries).to(dev)
    status = torch.full((n,), 9, dtype=torch.int32, device=dev)
    status[live] = 0
    far = pkg.knn_groups(cloud, K, queries=query, status=status, dist2=False)
    assert far.index.numel() > 2 ** 31 and far.dist2 is None
    assert torch.equal(far.index[live], small.index) and far.status[live].tolist() == [0, 0]
    assert (far.index[n - 2] == -1).all() and (far.index[1] == -1).all() and int(far.status.sum()) == 9 * (n - 2)


def test_a_cloud_that_ends_beyond_2_31_elements(pkg):
    dev = torch.device("cuda:0")
    _need_memory(dev)
    P, C, K = 64, 2, 3
    n = 2 ** 31 // (3 * P) + 3                                # 11184813 positions of 192 elements
    assert (n - 1) * 3 * P >= 2 ** 31 and n * 256 < 2 ** 32
    live = [0, n - 1]
    clouds = gr.patches(2, P, seed=33)
    t = torch.from_numpy(clouds).to(dev)
    small, nsmall = pkg.knn_groups(t, K, queries=C, offsets=True), pkg.point_normals(t, K, queries=C)
    assert gr.same_knn(type(small)(*[x.cpu().numpy() for x in small]), gr.knn(clouds, K, C)) is None
    assert gr.same_normals(type(nsmall)(*[x.cpu().numpy() for x in nsmall]), gr.normals(clouds, K, C)) is None
    cloud = torch.empty((n, P, 3), device=dev)                # never read but at the two live positions
    cloud[live] = t
    status = torch.ones(n, dtype=torch.int32, device=dev)
    status[live] = 0
    far, nfar = pkg.knn_groups(cloud, K, queries=C, status=status, offsets=True), pkg.point_normals(cloud, K, queries=C, status=status)
    assert cloud.numel() > 2 ** 31
    assert _same([x[live] for x in far], small) and _same([x[live] for x in nfar], nsmall)
    assert (far.index[n - 2] == -1).all() and not nfar.normals[n - 2].any() and int(far.status.sum()) == n - 2
