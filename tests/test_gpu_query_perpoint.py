"""GPU (-m gpu): the SIF-Net point query through the C ABI (csrc/query.hip, query_f32.hip), every output of every point against the float64 model of
tests/query_model.py in units of u S (u = 2^-24, S the output's own scale), on the cases of tests/query_cases.py.

Gates (tests/query_cases.py gate()): strict fp32 route GATE x e32, e32 = the float32 CPU oracle's worst error in the same units, measured per case family and kind of
output by tests/test_host_query_model.py (two correct float32 summation orders differ by a small multiple of each other's error; GATE = 8 as in
test_gpu_smplh_perjoint.py); split-f16 route + GATE x the split-operand emulation's measured error.  Never derived from the kernel's output.  Points within float32 reach
of a kink (query_model.excluded: at most 2 % of a case, none of the placed ones -- asserted on the CPU) are left out of the gradient gates only.  Terms: float64
atomics over float32 summands, query_model.term_gate.  Measured figures: tests/golden/query_perpoint.md; every test prints its own on failure."""
import ctypes as C

import numpy as np
import pytest

import query_cases as QC
import query_model as Q

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROUTES = ("split-f16", "fp32")


def cu(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def npy(t):
    return t.detach().cpu().numpy()


class GpuBackend:
    """the C ABI behind the interface of query_cases.evaluate(); route = vt_sifnet_set_precision per handle (fp32: also once through vt_maps::force_fp32)"""
    def __init__(self, route, force=False):
        from vistracker_amd import ops, _lib as L
        self.ops, self.L, self.route, self.force = ops, L, route, force
        self._nets, self._maps = {}, {}

    def net(self, case):
        k = (case.gain, tuple(case.cam))
        if k not in self._nets:
            self._nets[k] = self.ops.SifNetHandle(case.decoders(), cam=case.cam)
        n = self._nets[k]
        n.set_precision("split-f16" if (self.force or self.route == "split-f16") else "fp32")
        return n

    def maps(self, case, o=None):
        o = o or {}; k = (case.B, case.map_seed, case.gain, tuple(case.cam), bool(o.get("proj")), o.get("level", 0))
        if k not in self._maps:
            m = self.ops.FeatureMaps.from_nchw(case.maps()).set_act_level(o.get("level", 0))
            if self.force and self.route == "fp32":
                m.set_force_fp32(True)
            if o.get("proj"):
                m.build_projection(self.net(case))
            self._maps[k] = m
        return self._maps[k]

    def _args(self, case, o=None):
        L = self.L
        t = [cu(case.pts), cu(case.cc), cu(case.bc)]
        return t, (self.net(case).h, C.byref(self.maps(case, o).c), L.dptr(t[0]), L.dptr(t[1]), L.dptr(t[2]), case.B, case.N)

    def forward(self, case, heads, level=0):
        L = self.L; keep, a = self._args(case, dict(level=level))
        outs = [torch.full((case.B, k, case.N), float("nan"), device="cuda") if h in heads else None for h, k in enumerate(Q.HEAD_DIMS)]
        L.check(L.lib().vt_query_forward(*a, *[L.dptr(t) for t in outs], L.stream_ptr()))
        return {h: npy(outs[h]) for h in heads}

    def backward(self, case, g, level=0):
        L = self.L; keep, a = self._args(case, dict(level=level))
        gs = [cu(np.asarray(g[h], np.float32)) if h in g else None for h in range(5)]
        d = torch.full((case.B, case.N, 3), float("nan"), device="cuda")
        L.check(L.lib().vt_query_backward(*a, *[L.dptr(t) for t in gs], L.dptr(d), L.stream_ptr()))
        return npy(d)

    def _order(self, order):
        return None if order is None else cu(order)

    def human_loss(self, case, order, o):
        L = self.L; keep, a = self._args(case, o); lab = cu(case.labels); od = self._order(order)
        t = torch.zeros(2, dtype=torch.float64, device="cuda"); d = torch.full((case.B, case.N, 3), float("nan"), device="cuda")
        L.check(L.lib().vt_query_human_loss(*a, L.dptr(lab), L.dptr(od), QC.W_DFH, o.get("w_part", QC.W_PART), L.dptr(d), L.dptr(t), L.stream_ptr()))
        return npy(d), npy(t)

    def human_step(self, case, order, o, acc):
        L = self.L; keep, a = self._args(case, o); lab = cu(case.labels); od = self._order(order)
        t = torch.zeros(2, dtype=torch.float64, device="cuda"); ta = torch.zeros(1, dtype=torch.float64, device="cuda")
        d = cu(case.base) if acc else torch.full((case.B, case.N, 3), float("nan"), device="cuda")
        L.check(L.lib().vt_query_human_step(*a, L.dptr(lab), L.dptr(od), QC.W_DFH, QC.W_PART, int(acc), QC.W_ACCEL, L.dptr(ta), L.dptr(d), L.dptr(t), L.stream_ptr()))
        return npy(d), npy(t), float(npy(ta)[0])

    def object_loss(self, case, o):
        L = self.L; keep, a = self._args(case, o); occ = cu(case.occ)
        t = torch.zeros(2, dtype=torch.float64, device="cuda"); d = torch.full((case.B, case.N, 3), float("nan"), device="cuda")
        L.check(L.lib().vt_query_object_loss(*a, L.dptr(occ), QC.W_OBJ, L.dptr(d), L.dptr(t), L.stream_ptr()))
        return npy(d), npy(t)

    def project_step(self, case, idx, thr, o):
        L = self.L; keep, a = self._args(case, o)
        out = torch.full((case.B, case.N, 3), float("nan"), device="cuda"); tgt = torch.full((case.B, case.N), float("nan"), device="cuda")
        L.check(L.lib().vt_query_project_step(*a, int(idx), float(thr), L.dptr(out), L.dptr(tgt), L.stream_ptr()))
        return npy(out), npy(tgt)


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in QC.all_cases()}


@pytest.fixture(scope="module", params=ROUTES)
def backend(request):
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return GpuBackend(request.param)


def check(case, be, fused_opts=None, level=0):
    recs, terms, exact = QC.evaluate(case, be, route=be.route, fused_opts=fused_opts, level=level)
    lines, bad = [], []
    for r in recs:
        g = QC.gate(case.family, r.kind, be.route, r.level); w = r.worst()
        lines.append("%-10s %-9s %-6s %-58s worst %.4g u S  gate %.4g  (%.3g of the gate)" % (case.name, be.route, r.kind, r.op, w, g, w / g))
        if not w <= g:
            bad.append(lines[-1])
        if case.family == "tiles":                        # first and last point of every tile and of every frame, one by one
            for b in range(case.B):
                for n in QC.tile_edges(case.N):
                    idx = (b, slice(None), n) if r.kind == "value" else (b, n)
                    if r.gated[idx].any() and not r.units[idx][r.gated[idx]].max() <= g:
                        bad.append("%s: frame %d point %d: %.4g u S > %.4g" % (r.op, b, n, r.units[idx].max(), g))
    for name, err, g in terms:
        lines.append("%-10s %-9s term   %-58s error %.4g  gate %.4g  (%.3g of the gate)" % (case.name, be.route, name, err, g, err / g))
        if not err <= g:
            bad.append(lines[-1])
    for what, ok in exact:
        if not ok:
            bad.append("%s %s: NOT MET: %s" % (case.name, be.route, what))
    print("\n".join(lines))
    assert not bad, "\n".join(bad) + "\n--- all figures ---\n" + "\n".join(lines)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 150])
def test_tile_edges_every_head_and_the_pairs(cases, backend, N):
    """N around the 64-point tile, B = 2 with a crop and body centre per frame; forward with five and with two outputs, backward with every head alone (G = 1) and the
    pairs (df, parts), (pca, vis) (G = 2), one head's gradients 2^10 times the other's, each head gated on its own scale"""
    check(cases["tiles-N%d" % N], backend)


def test_upstream_gradients_over_30_binades(cases, backend):
    """2^-20 .. 2^10 per point and per head within one tile (the GO_EXP normalisation); exactly zero next to 2^10 gives exactly zero"""
    check(cases["goexp"], backend)


def test_image_and_grid_borders(cases, backend):
    """nx, ny exactly -1, +1 and a float32 step outside; triplane coordinates on the first / last texel and beyond; df == 5.0 bit for bit outside, no df gradient there"""
    check(cases["borders"], backend)


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name", ["tiles-N65", "tiles-N150", "goexp", "borders"])
def test_plain_forward_and_backward_at_range_levels_1_and_2(cases, backend, name, level):
    """vt_query_forward / vt_query_backward pick every head's weights, biases and output scale of vt_maps::act_level (the strict-fp32 route ignores it): all five heads,
    G = 1 and G = 2, the tile edges, the 30 binades of upstream gradients and the placed borders at the rescaled operand scale -- an exact power-of-two rescaling, so the
    same model and the same gate as at level 0"""
    check(cases[name], backend, level=level)


FUSED_OPTS = [dict(order=od, proj=pj, level=lv) for od, pj, lv in (("identity", False, 0), ("random", False, 0), ("reversed", True, 0), ("identity", True, 0),
                                                                  ("random", False, 1), ("random", True, 1), ("reversed", False, 2), ("identity", True, 2))]


def test_fused_objectives_order_projection_levels(cases, backend):
    """vt_query_human_loss / vt_query_object_loss / vt_query_project_step: clamp edges, the three orders, the hoisted projection on and off, the range levels 0, 1, 2
    (exact power-of-two rescaling: the same gate) -- every variant against the MODEL, not against each other; vt_query_human_step (split-f16 route only) with
    accumulate 0 / 1 and the acceleration term"""
    opts = [dict(o) for o in FUSED_OPTS]
    if backend.route == "split-f16":
        opts[0]["step"] = True; opts[3]["step"] = True
    check(cases["fused"], backend, opts)


def test_large_activations_need_level_1(cases, backend):
    """sifnet_decoders(gain = 8): the last hidden layer beyond level 0's range (asserted on the CPU), run at level 1 and 2"""
    check(cases["gain"], backend, [dict(order="random", proj=False, level=1), dict(order="identity", proj=True, level=1), dict(order="reversed", proj=True, level=2)])


def test_force_fp32_is_the_strict_route(cases):
    """vt_maps::force_fp32 on a split-f16 handle: the strict-fp32 gates"""
    be = GpuBackend("fp32", force=True)
    check(cases["tiles-N65"], be); check(cases["fused"], be, [dict(order="random", proj=False, level=0)])
