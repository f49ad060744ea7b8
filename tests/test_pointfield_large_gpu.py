"""The offset-field kernels beyond the 32-bit element range (include/tsdf_pointfield.h: all global indexing is in 64
bits): one call whose bfloat16 field ends beyond element 2^31, written by the encoder and read by the decoder, and one
whose cloud does.  The positions at both ends are compared with the same positions in a small call, which is compared with
the numpy restatement (tests/pointfield_ref.py).  The positions that need no check carry a non-zero input status and are
not read."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointfield_ref as pr  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _need_memory(dev, gib):
    free, _ = torch.cuda.mem_get_info(dev)
    assert free > gib * 2 ** 30, f"this test needs {gib} GiB of device memory"


def _same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype is torch.float32 else x.view(torch.int16) if x.element_size() == 2 else x,
                           y.view(torch.int32) if y.dtype is torch.float32 else y.view(torch.int16) if y.element_size() == 2 else y)
               for x, y in zip(a, b))


def _host(b):
    return type(b)(*[t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype is torch.bfloat16 else t.cpu().numpy() for t in b])


def _small(pkg, dev, clouds, joints, K, radius, M):
    """The two live positions alone, held to the restatement: (encode's batch, decode's batch)."""
    c, j = torch.from_numpy(clouds).to(dev), torch.from_numpy(joints).to(dev)
    enc = pkg.point_fields(c, j, K, radius=radius, dtype=torch.bfloat16)
    want = pr.encode(clouds, joints, K, radius)
    assert pr.same_field(_host(enc), want, "bfloat16") is None
    dec = pkg.field_joints(c, enc.field, radius=radius, points=M)
    assert pr.same_joints(_host(dec), pr.decode(clouds, pr.widen(pr.narrow(want.field, "bfloat16"), "bfloat16"), M, radius)) is None
    assert (dec.weight > 0).any()
    return enc, dec


def test_a_bfloat16_field_that_ends_beyond_2_31_elements(pkg):
    dev = torch.device("cuda:0")
    _need_memory(dev, 8)
    P, J, K, M, radius = 1024, 21, 64, 25, 25.0
    n = 2 ** 31 // (4 * J * P) + 2                            # 24968 positions of 86016 elements
    assert (n - 1) * 4 * J * P >= 2 ** 31
    live = [0, n - 1]
    clouds = pr.random_clouds(2, P, seed=31, scale=20.0)
    joints = pr.joints_near(clouds, J, seed=32, spread=5.0)
    enc, dec = _small(pkg, dev, clouds, joints, K, radius, M)
    cloud = torch.zeros((n, P, 3), device=dev)
    joint = torch.zeros((n, J, 3), device=dev)
    cloud[live], joint[live] = torch.from_numpy(clouds).to(dev), torch.from_numpy(joints).to(dev)
    status = torch.full((n,), 9, dtype=torch.int32, device=dev)
    status[live] = 0
    far = pkg.point_fields(cloud, joint, K, radius=radius, dtype=torch.bfloat16, status=status)
    assert far.field.numel() > 2 ** 31
    assert _same([t[live] for t in far], enc) and int(far.status.sum()) == 9 * (n - 2)
    assert not far.field[n - 2].any() and not far.field[1].any() and not far.valid[1:n - 1].any()
    back = pkg.field_joints(cloud, far.field, radius=radius, points=M, status=status)
    assert _same([t[live] for t in back], dec) and not back.joints[n - 2].any() and not back.weight[1:n - 1].any()


def test_a_cloud_that_ends_beyond_2_31_elements(pkg):
    dev = torch.device("cuda:0")
    _need_memory(dev, 20)
    P, J, K, M, radius = 64, 1, 8, 5, 25.0
    n = 2 ** 31 // (3 * P) + 3                                # 11184813 positions of 192 elements
    assert (n - 1) * 3 * P >= 2 ** 31 and n * 256 < 2 ** 32
    live = [0, n - 1]
    clouds = pr.random_clouds(2, P, seed=33, scale=20.0)
    joints = pr.joints_near(clouds, J, seed=34, spread=5.0)
    enc, dec = _small(pkg, dev, clouds, joints, K, radius, M)
    cloud = torch.empty((n, P, 3), device=dev)                # never read but at the two live positions
    joint = torch.zeros((n, J, 3), device=dev)
    cloud[live], joint[live] = torch.from_numpy(clouds).to(dev), torch.from_numpy(joints).to(dev)
    status = torch.ones(n, dtype=torch.int32, device=dev)
    status[live] = 0
    far = pkg.point_fields(cloud, joint, K, radius=radius, dtype=torch.bfloat16, status=status)
    assert cloud.numel() > 2 ** 31
    assert _same([t[live] for t in far], enc) and int(far.status.sum()) == n - 2 and not far.field[n - 2].any()
    back = pkg.field_joints(cloud, far.field, radius=radius, points=M, status=status)
    assert _same([t[live] for t in back], dec) and not back.joints[n - 2].any() and int((back.weight != 0).sum()) == int((dec.weight != 0).sum())
