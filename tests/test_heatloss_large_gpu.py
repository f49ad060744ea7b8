"""The heatloss kernels beyond the 32-bit range (include/tsdf_heatloss.h): n = 49 frames of 21 joints at R = 128 in bfloat16
are 2,157,969,408 elements and 4,315,938,816 bytes — past element 2^31 and past byte 2^32; a prediction and a gradient
of that size are about 9 GB at the peak.  For all four entries the last two frames, which hold the crossing (joint 16 of
the last frame starts at element 2^31) and everything beyond it, must come out bit for bit as those of the same two
frames as a compact batch of two (what tests/test_heatloss_gpu.py checks against the restatement at R = 128), and the
guards after the ends must survive."""
import importlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def bits(t):
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def test_all_four_entries_beyond_2_31_elements_and_2_32_bytes(pkg):
    V = importlib.import_module(pkg.__name__ + ".voxelize")
    L = pkg._lib.load_heatloss()
    n, J, R, BF16 = 49, 21, 128, 2
    count = n * J * R ** 3
    assert count == 2_157_969_408 > 2 ** 31 and 2 * count == 4_315_938_816 > 2 ** 32
    assert ((n - 1) * J + 16) * R ** 3 == 2 ** 31         # joint 16 of the last frame starts at element 2^31, byte 2^32
    dev = torch.device("cuda:0")
    free, _ = torch.cuda.mem_get_info(dev)
    assert free > 10 * 2 ** 30, "this test needs about 9 GB of device memory"
    rng = np.random.default_rng(49)
    u = torch.from_numpy(rng.uniform(0.02, 0.98, (n, J, 3)).astype(np.float32)).to(dev)
    u[n - 1, 3] = float("nan")                    # an invalid joint in the compared part, a bad frame before it
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    status[5] = 1
    w = torch.from_numpy(rng.standard_normal((n, J)).astype(np.float32)).to(dev)
    gu = torch.from_numpy(rng.standard_normal((n, J, 3)).astype(np.float32)).to(dev)
    pbuf = torch.empty((count + 64,), dtype=torch.bfloat16, device=dev)
    pbuf.normal_()                                 # filled on the device
    pred = pbuf[:count].view(n, J, R, R, R)
    gbuf = torch.full((count + 64,), float("nan"), dtype=torch.bfloat16, device=dev)
    grad = gbuf[:count].view(n, J, R, R, R)
    last = slice(n - 2, n)
    cpred, cu, cstatus, cw, cgu = (t[last].clone() for t in (pred, u, status, w, gu))

    def outputs(m):
        f64 = torch.full((m * J * 6 + 64,), float("nan"), dtype=torch.float64, device=dev)
        i32 = torch.full((m * J + 64,), -7, dtype=torch.int32, device=dev)
        f32 = torch.full((m * J * 3 + 64,), float("nan"), device=dev)
        return f64, i32, f32

    def guards_intact(f64, i32, f32, m):
        return bool(torch.isnan(f64[m * J * 6:]).all()) and bool((i32[m * J:] == -7).all()) and bool(torch.isnan(f32[m * J * 3:]).all())

    def run(p, lab, st, ww, g, out, m, layout):
        f64, i32, f32 = outputs(m)
        sse, stats = f64[:m * J], f64[m * J:m * J * 6]
        lay = pkg._lib.LAYOUTS[layout]
        V._call(dev, L.tsdf_heat_sse_hip, [p.data_ptr(), BF16, lab.data_ptr(), st.data_ptr(), m, J, R, 1.7, lay, None,
                                           sse.data_ptr(), i32.data_ptr()], 9)
        V._call(dev, L.tsdf_heat_sse_grad_hip, [p.data_ptr(), BF16, lab.data_ptr(), st.data_ptr(), ww.data_ptr(), m, J, R, 1.7, lay,
                                                None, out.data_ptr()], 10)
        torch.cuda.synchronize()
        loss_grad = out[m - 2:].clone()
        V._call(dev, L.tsdf_soft_argmax_hip, [p.data_ptr(), BF16, m, J, R, 2.0, lay, None, f32.data_ptr(), stats.data_ptr()], 7)
        V._call(dev, L.tsdf_soft_argmax_grad_hip, [p.data_ptr(), BF16, stats.data_ptr(), g.data_ptr(), m, J, R, 2.0, lay, None,
                                                   out.data_ptr()], 9)
        torch.cuda.synchronize()
        assert guards_intact(f64, i32, f32, m)
        return (sse.view(m, J)[m - 2:], i32[:m * J].view(m, J)[m - 2:], loss_grad, f32[:m * J * 3].view(m, J, 3)[m - 2:],
                stats.view(m, J, 5)[m - 2:], out[m - 2:])

    for layout in ("czyx", "cxyz"):
        big = run(pred, u, status, w, gu, grad, n, layout)
        assert bool(torch.isnan(gbuf[count:]).all())
        assert not bool(torch.isnan(grad[0]).any()) and bool(grad[0].any())           # and the front was written too
        compact = run(cpred, cu, cstatus, cw, cgu, torch.empty_like(cpred), 2, layout)
        for name, x, y in zip(("sse", "valid", "loss gradient", "u", "stats", "soft-argmax gradient"), big, compact):
            assert torch.equal(bits(x.contiguous()), bits(y.contiguous())), (layout, name)
        sse, valid, lgrad, su, stats, sgrad = compact
        assert int(valid.sum()) == 2 * J - 1 and float(sse[1, 3]) == 0.0 and not bool(bits(lgrad[1, 3]).any())
        assert bool((sse[valid.bool()] > R ** 3 / 2).all())                            # standard-normal values: about R^3 each
        assert bool(((su > 0.4) & (su < 0.6)).all()) and bool((stats[..., 1] >= 1).all()) and bool(sgrad.any())
