"""GPU (-m gpu): the silhouette kernels of csrc/sil.hip through the C ABI, per pixel and per vertex, on the cases of tests/sil_cases.py.

Forward: image and owner map equal to the float32 CPU oracle's pixel for pixel; the only pixels left out are those where oracle and model were found to DIFFER
(sil_cases.reference 'skip': each shown contested, at most 0.5 % of the covered ones, by tests/test_host_sil_model.py -- a handful per case), none in the lattice
cases at 64, 192 and 256, the layers cases (gaps >= 1e-4) and the sliver cases.
Backward: every vertex component within GATE x E32 x u S (+ the rounding Q of the fixed-point accumulators) of the model on the oracle's owner map; S = 0 -> exactly
0; two runs bit-equal.  E32 is the float32 oracle's own error on the same case in the same units (sil_cases.E32, measured on the CPU), GATE = 8; nothing is derived from the kernel's
output.  vt_sil_step: bit-equal to the three separate calls, d_image bit-equal to the model's float32 evaluation (the library is built with -ffp-contract=off), the
term within 1e-12 relative + tiles x 2^-35 of the float64 model.  Sweep masks, read out of the workspace, bit for bit.  Measured figures: tests/golden/sil_perpixel.md."""
import numpy as np
import pytest

import sil_cases as SC
import sil_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = SC.all_cases()
STEP_CASES = [c for c in CASES if c.d_image is None and (c.family == "inside" or c.name in ("cut-64", "cut-192", "cut-320", "lattice-64", "slivers-192", "counts-64-nf17"))]


def cu(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def npy(t):
    return t.detach().cpu().numpy()


class Gpu:
    def __init__(self, c):
        from vistracker_amd import _lib as L
        assert torch.cuda.is_available(), "GPU tests need the MI355X box"
        self.L, self.lib, self.c = L, L.lib(), c
        self.v, self.f, self.k = cu(c.verts), cu(c.faces), cu(c.K)
        n = self.lib.vt_sil_workspace_floats(c.B, c.NV, c.NF, c.size)
        self.ws = torch.full((n + (n & 1),), float("nan"), device="cuda")          # poisoned: no call may depend on what the workspace held
        self.st = L.stream_ptr()

    def forward(self):
        c, L = self.c, self.L
        img = torch.full((c.B, c.size, c.size), float("nan"), device="cuda"); fi = torch.full((c.B, c.size, c.size), -7, dtype=torch.int32, device="cuda")
        L.check(self.lib.vt_sil_forward(L.dptr(self.v), c.B, c.NV, L.dptr(self.f), c.NF, L.dptr(self.k), c.size, L.dptr(img), L.dptr(fi), L.dptr(self.ws), self.st))
        self.fi = fi
        return npy(img), npy(fi)

    def backward(self, fi, dimg):
        c, L = self.c, self.L
        self.dimg = cu(dimg); fi = cu(fi.astype(np.int32))
        dv = torch.full((c.B, c.NV, 3), float("nan"), device="cuda")
        L.check(self.lib.vt_sil_backward(L.dptr(self.v), c.B, c.NV, L.dptr(self.f), c.NF, L.dptr(self.k), c.size, L.dptr(fi), L.dptr(self.dimg), c.eps, L.dptr(self.ws),
                                         L.dptr(dv), self.st))
        return npy(dv)

    def masks(self):
        c = self.c; s, wpl = c.size, c.size // 64
        w = npy(self.ws.view(torch.int64)).view(np.uint64)
        o = c.B * s * s; n = c.B * s * wpl
        return w[o:o + n].reshape(c.B, s, wpl), w[o + n:o + 2 * n].reshape(c.B, s, wpl)


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_forward_and_backward(c):
    r = SC.reference(c); g = Gpu(c)
    img, fi = g.forward()
    skip = r["skip"]
    bad = ((fi != r["fi"]) | (img != r["img"])) & ~skip
    if not c.asserted:
        print(f"{c.name}: {int(bad.sum())} pixels differ from the oracle (gaps {SC.NARROW_GAPS}: printed, not asserted)")
    else:
        msg = [(tuple(p), int(fi[tuple(p)]), int(r["fi"][tuple(p)]), float(r["fw"][p[0]]["z1"][p[1], p[2]]), float(r["fw"][p[0]]["z2"][p[1], p[2]])) for p in np.argwhere(bad)[:8]]
        assert not bad.any(), f"{c.name}: {int(bad.sum())} pixels (pixel, kernel owner, oracle owner, model depths): {msg}"
    # backward on the ORACLE's owner map (the forward kernels have run: the workspace holds their face records)
    dv = g.backward(r["fi"], r["dimg"])
    assert np.isfinite(dv).all(), c.name
    u = M.units(dv, r["grad"], r["S"], r["Q"])
    assert (dv[r["S"] == 0] == 0).all(), c.name
    i = np.unravel_index(np.argmax(u), u.shape)
    print(f"{c.name}: worst |kernel - model| = {u[i]:.1f} u S at (frame, vertex, component) {i}; gate {SC.gate(c):.0f}; ratio {u[i] / SC.gate(c):.4f}")
    if c.asserted:
        assert u[i] <= SC.gate(c), (c.name, i, float(u[i]), float(dv[i]), float(r["grad"][i]), float(r["S"][i]))
    assert np.array_equal(dv, g.backward(r["fi"], r["dimg"])), "two runs on the same inputs differ"
    if c.size in (64, 192, 320) and c.family in ("inside", "cut", "lattice"):
        row, col = g.masks()
        for b in range(c.B):
            mr, mc = M.sweep_masks(r["fi"][b], r["dimg"][b])
            assert np.array_equal(row[b], M.pack_words(mr)) and np.array_equal(col[b], M.pack_words(mc)), (c.name, b)


@pytest.mark.parametrize("c", STEP_CASES, ids=repr)
def test_step_equals_the_separate_calls_and_the_model(c):
    r = SC.reference(c); g = Gpu(c); L, lib = g.L, g.lib
    B, s = c.B, c.size
    kp, rf, oc = cu(c.keep), cu(c.ref), cu(c.occ)
    img, fi = g.forward(); imgd = cu(img)
    term = torch.zeros(1, dtype=torch.float64, device="cuda"); per = torch.full((B,), float("nan"), device="cuda"); dimg = torch.full((B, s, s), float("nan"), device="cuda")
    L.check(lib.vt_sil_mask_loss(L.dptr(imgd), L.dptr(kp), L.dptr(rf), L.dptr(oc), B, s, c.gscale, term.data_ptr(), L.dptr(per), L.dptr(dimg), g.st))
    term16 = torch.zeros(1, dtype=torch.float64, device="cuda"); dimg16 = torch.full((B, s, s), float("nan"), device="cuda")
    L.check(lib.vt_sil_mask_loss(L.dptr(imgd), L.dptr(kp), L.dptr(rf), L.dptr(oc), B, s, c.gscale, term16.data_ptr(), None, L.dptr(dimg16), g.st))
    d_sep = npy(dimg); dv_sep = g.backward(fi, d_sep)
    # the model's float32 evaluation on the kernel's own image (equal to the oracle's outside contested pixels: test_forward_and_backward)
    d_mod, t_mod, per_mod = M.mask_term(img, c.keep, c.ref, c.occ, c.gscale)
    assert np.array_equal(d_sep.view(np.uint32), d_mod.view(np.uint32)) and np.array_equal(npy(dimg16).view(np.uint32), d_mod.view(np.uint32))
    assert np.array_equal(npy(per), per_mod.astype(np.float32))
    tiles = (s // 64) ** 2
    for t in (term, term16):
        assert abs(float(t.item()) - t_mod) <= 1e-12 * t_mod, (float(t.item()), t_mod)
    g2 = Gpu(c); fi2 = torch.full((B, s, s), -7, dtype=torch.int32, device="cuda"); dimg2 = torch.full((B, s, s), float("nan"), device="cuda")
    for rep in range(2):
        dv = torch.full((B, c.NV, 3), float("nan"), device="cuda"); t2 = torch.zeros(1, dtype=torch.float64, device="cuda")
        L.check(lib.vt_sil_step(L.dptr(g2.v), B, c.NV, L.dptr(g2.f), c.NF, L.dptr(g2.k), s, L.dptr(kp), L.dptr(rf), L.dptr(oc), c.gscale, c.eps, t2.data_ptr(), L.dptr(fi2),
                                L.dptr(dimg2), L.dptr(g2.ws), L.dptr(dv), g2.st))
        assert np.array_equal(npy(fi2), fi) and np.array_equal(npy(dimg2).view(np.uint32), d_mod.view(np.uint32)), (c.name, rep)
        assert np.array_equal(npy(dv).view(np.uint32), dv_sep.view(np.uint32)), (c.name, rep, float(np.abs(npy(dv) - dv_sep).max()))
        assert abs(float(t2.item()) - t_mod) <= 1e-12 * t_mod + tiles * 2.0 ** -35, (c.name, rep, float(t2.item()), t_mod)


@pytest.mark.parametrize("size", (64, 192))
def test_triplane_equals_the_oracle(size):
    from oracle import oracle as O
    from vistracker_amd import _lib as L
    c = [x for x in CASES if x.name == f"inside-{size}"][0]
    verts = c.verts * np.float32(1.6); center = verts.mean(1) + np.float32(0.01)
    want = O.triplane_render(verts, c.faces, center, size)
    B = c.B; v, f, ce = cu(verts), cu(c.faces), cu(center.astype(np.float32))
    n = L.lib().vt_sil_workspace_floats(3 * B, c.NV, c.NF, size)
    ws = torch.full((n,), float("nan"), device="cuda"); masks = torch.full((B, 3, size, size), float("nan"), device="cuda")
    fi = torch.empty((B, 3, size, size), dtype=torch.int32, device="cuda")
    L.check(L.lib().vt_triplane_render(L.dptr(v), L.dptr(ce), B, c.NV, L.dptr(f), c.NF, size, L.dptr(masks), L.dptr(fi), L.dptr(ws), L.stream_ptr()))
    assert 0.02 < want.mean() < 0.9 and int((npy(masks) != want).sum()) == 0


@pytest.mark.parametrize("size,nf", [(0, 5), (100, 5), (32768, 5), (64, 0)])
def test_bad_sizes_are_refused_before_any_launch(size, nf):
    from vistracker_amd import _lib as L
    lib = L.lib(); st = L.stream_ptr()
    B, NV = 1, 8
    v = torch.zeros(B, NV, 3, device="cuda"); f = torch.zeros(8, 3, dtype=torch.int32, device="cuda"); k = torch.zeros(B, 9, device="cuda")
    a = torch.full((64 * 64 * 3,), 3.0, device="cuda"); ai = torch.full((64 * 64 * 3,), 3, dtype=torch.int32, device="cuda"); ws = torch.full((1 << 16,), 3.0, device="cuda")
    dv = torch.full((B, NV, 3), 3.0, device="cuda"); term = torch.zeros(1, dtype=torch.float64, device="cuda")
    calls = {
        "vt_sil_forward": lambda: lib.vt_sil_forward(L.dptr(v), B, NV, L.dptr(f), nf, L.dptr(k), size, L.dptr(a), L.dptr(ai), L.dptr(ws), st),
        "vt_sil_step": lambda: lib.vt_sil_step(L.dptr(v), B, NV, L.dptr(f), nf, L.dptr(k), size, L.dptr(a), L.dptr(a), L.dptr(k), 1.0, 1e-4, term.data_ptr(), L.dptr(ai), L.dptr(a),
                                               L.dptr(ws), L.dptr(dv), st),
        "vt_sil_backward": lambda: lib.vt_sil_backward(L.dptr(v), B, NV, L.dptr(f), nf, L.dptr(k), size, L.dptr(ai), L.dptr(a), 1e-4, L.dptr(ws), L.dptr(dv), st),
        "vt_triplane_render": lambda: lib.vt_triplane_render(L.dptr(v), L.dptr(k), B, NV, L.dptr(f), nf, size, L.dptr(a), L.dptr(ai), L.dptr(ws), st),
    }
    for name, call in calls.items():
        assert call() != 0, name
        assert name in lib.vt_last_error().decode() and "bad argument" in lib.vt_last_error().decode(), (name, lib.vt_last_error())
    torch.cuda.synchronize()
    assert (dv == 3.0).all() and (ws == 3.0).all() and (a == 3.0).all() and (ai == 3).all()          # nothing was launched: no output or workspace word was touched
