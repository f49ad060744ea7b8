"""The heatmap kernels beyond the 32-bit range (include/tsdf_heatmap.h): n = 49 frames of 21 joints at R = 128 in bfloat16
are 2,157,969,408 elements and 4,315,938,816 bytes — past element 2^31 and past byte 2^32; about 4.5 GB at the peak.  The
last two frames' volumes, which hold the crossing (joint 16 of the last frame starts at element 2^31) and everything
beyond it, must be those of the same joints encoded as a batch of two; the
guard after the end must survive; and the decode of the big buffer must find in them what it finds in the compact one."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def test_encode_and_decode_beyond_2_31_elements_and_2_32_bytes(pkg):
    n, J, R = 49, 21, 128
    count = n * J * R ** 3
    assert count == 2_157_969_408 > 2 ** 31 and 2 * count == 4_315_938_816 > 2 ** 32
    assert ((n - 1) * J + 16) * R ** 3 == 2 ** 31         # joint 16 of the last frame starts at element 2^31, byte 2^32
    dev = torch.device("cuda:0")
    free, _ = torch.cuda.mem_get_info(dev)
    assert free > 5 * 2 ** 30, "this test needs about 4.5 GB of device memory"
    rng = np.random.default_rng(49)
    u = torch.from_numpy(rng.uniform(0.02, 0.98, (n, J, 3)).astype(np.float32)).to(dev)
    u[n - 1, 3] = float("nan")                    # an invalid joint in the compared part, a bad frame before it
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    status[5] = 1
    buf = torch.full((count + 64,), float("nan"), dtype=torch.bfloat16, device=dev)
    out = buf[:count].view(n, J, R, R, R)
    for layout in ("czyx", "cxyz"):
        heat, valid = pkg.joint_heatmaps(u, R, 1.7, layout=layout, dtype=torch.bfloat16, status=status, out=out, return_valid=True)
        small, svalid = pkg.joint_heatmaps(u[n - 2:].contiguous(), R, 1.7, layout=layout, dtype=torch.bfloat16,
                                           status=status[n - 2:].contiguous(), return_valid=True)
        torch.cuda.synchronize()
        assert heat is out and bool(torch.isnan(buf[count:]).all())
        assert torch.equal(heat[n - 2:].view(torch.int16), small.view(torch.int16))
        assert torch.equal(valid[n - 2:], svalid) and int(svalid.sum()) == 2 * J - 1
        assert not bool(heat[n - 1, 3].any()) and float(small[:, :3].max()) > 0.3
        assert not bool(torch.isnan(heat[0]).any()) and bool(heat[0].any())          # and the front was written too
        big = pkg.heatmap_joints(heat, layout=layout, radius=2)
        compact = pkg.heatmap_joints(small, layout=layout, radius=2)
        torch.cuda.synchronize()
        for x, y in zip(big, compact):
            assert torch.equal(x[n - 2:].view(torch.int32), y.view(torch.int32))
        ok = svalid.bool()
        assert bool((compact.arg[ok] >= 0).all()) and bool((compact.peak[ok] > 0.3).all())
        # The window is centred on the argmax voxel i*, |c - i*| <= 0.5, and cuts weights that are symmetric about c: the
        # centre of mass lies between i* and c.  bfloat16 weights are off by 2^-9 relative, each at most 2 voxels from i*.
        err = (compact.u - u[n - 2:]).abs()[ok]
        assert float(err.max()) <= (0.5 + 2.0 ** -6) / R + 2.0 ** -23
