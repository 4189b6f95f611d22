"""CPU: the conditions that tests/test_gpu_collide.py relies on, from the float64 model (tests/collide_model.py) and the cases (tests/collide_cases.py) alone, and the
product's header collide_geom.h compiled for the host (system C compiler, -ffp-contract=off, a stand-alone driver that walks the pairs the way the kernels do) against
the gates of the GPU test: a fault of the geometry shows here without a GPU."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import collide_cases as C
import collide_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIT_FRAMES = (0, 2, 4, 5)


def test_the_two_model_gradients_agree():
    """analytic d/dt against torch float64 autograd through the whole value (the circumcentre, normal and radius of the moved object triangles included)"""
    worst = 0.0
    for name, mc in [("pairs", 8), ("order_700", 8), ("order_257", 2), ("fit_like", 8)] + C.FAMILY["blocks"]:
        for b, r in enumerate(C.reference(name, mc)):
            if r["pairs"] == 0:
                assert r["V"] == 0 and not r["g"].any(); continue
            V, g = M.value_autograd(r["S_kept"], r["O_kept"], C.SIGMA)
            assert abs(V - r["V"]) <= 1e-13 * V, (name, b)
            if np.abs(g).max() > 0:
                e = float(np.abs(g - r["g"]).max() / np.abs(g).max()); worst = max(worst, e); assert e <= 1e-10, (name, mc, b, e)
    print("analytic against autograd: worst relative difference %.2e (gate 1e-10)" % worst)


def test_every_planted_frame_takes_its_branch():
    ref = C.reference("pairs"); census = {}
    for name, b in C.PLANTED.items():
        r = ref[b]; assert len(r["box_pairs"]) == 1 and not r["undecided"].any(), name
        if name in ("axis", "phi_under", "phi_over", "apex", "linear"):
            assert r["pairs"] == 1 and r["margin"][0] > 50 * M.tau(r["S_kept"], r["O_kept"])[0], name
            s = {k: v[0, 0] for k, v in r["terms"]["sides"][0].items() if k != "r"}                     # object vertex 0 in the SMPL triangle's cone
            census[name] = "x %.4g Phi %.6g rho %.4g Dn %.4g" % (s["x"], s["Phi"], s["rho"], s["Dn"])
            if name == "axis": assert s["code"] == M.QUAD and s["rho"] == 0 and s["value"] > 0 and (r["terms"]["sides"][0]["rho"][0, 1:] > 0).all()
            if name == "phi_under": assert s["code"] == M.QUAD and 1 - 2.0 ** -11 < s["Phi"] < 1 - 2.0 ** -13
            if name == "phi_over": assert s["code"] == M.OUTSIDE and 1 + 2.0 ** -13 < s["Phi"] < 1 + 2.0 ** -11
            if name == "apex": assert s["code"] == M.APEX and s["x"] >= C.SIGMA and s["Dn"] <= 0
            if name == "linear": assert s["code"] == M.LINEAR and s["x"] <= -C.SIGMA and s["value"] > 0
            if name in ("apex", "linear"):
                e = np.linalg.norm(np.roll(r["S_kept"][0], 1, 0) - r["S_kept"][0], axis=1); assert (e >= 1).all() and (e <= 2).all(), e
        else:
            assert r["pairs"] == 0 and r["V"] == 0
            if name == "coplanar": assert r["coplanar"][0] and r["margin"][0] >= 0
            if name.startswith("zero_area"): assert r["degenerate"][0]
            if name == "separated": assert r["margin"][0] < -1e-3 and not r["coplanar"][0]
    for k, v in census.items():
        print("planted %-10s frame %3d: %s" % (k, C.PLANTED[k], v))


def test_undecided_pairs():
    """order, blocks and the planted frames of pairs: no undecided box-overlapping pair.  Random pairs frames with one: at most 1 % -- the only frames the GPU test
    leaves out.  fit_like: counted."""
    for name, mc in C.FAMILY["order"] + C.FAMILY["blocks"]:
        assert sum(int(r["undecided"].sum()) for r in C.reference(name, mc)) == 0, name
    ref = C.reference("pairs"); und = [b for b, r in enumerate(ref) if r["undecided"].any()]
    assert not set(und) & set(C.PLANTED.values())
    hit = sum(r["pairs"] for r in ref); rnd = len(ref) - len(C.PLANTED)
    print("pairs: %d of %d frames collide, %d frames have overlapping boxes, undecided frames %s = %.2f %% of the random frames" % (hit, len(ref), sum(len(r["box_pairs"]) for r in ref), und, 100.0 * len(und) / rnd))
    assert len(und) <= 0.01 * rnd and 0.15 * rnd < hit < 0.3 * rnd
    for b, r in enumerate(C.reference("fit_like")):
        s = M.slack(r, 8)
        print("fit_like frame %d: %d pairs on %d object faces, %d box-overlapping pairs, %d undecided; they can move the count to %d..%d, V by %.2e of V, dV/dt by %.2e of its largest component"
              % (b, r["pairs"], r["n_f"], len(r["box_pairs"]), int(r["undecided"].sum()), s[2], s[3], s[0] / r["V"], s[1].max() / np.abs(r["g"]).max()))
        assert r["pairs"] > 200


def test_order_case_shapes_and_subset_gaps():
    """the planted indices, the candidate counts, the two empty frames, and: any two subsets of the same size of a frame's colliding pairs differ in V by more than 100
    value gates, so the value names the subset that was kept"""
    seen = set(); least = np.inf
    for name in C.ORDER_CASES:
        c = C.case(name); NFs = len(c["sf"]); full = C.reference(name, 64)
        for b, r in enumerate(full):
            hits = list(r["box_pairs"][r["collide"], 1]); assert hits == c["planted"][b] and (b in HIT_FRAMES) == (len(hits) > 0), (name, b)
            seen |= set(hits)
        assert full[1]["n_cand"] == 0 and full[3]["n_cand"] > 200 and full[3]["pairs"] == 0
        assert all((full[b]["n_cand"] > 256) == (NFs > 500) and full[b]["n_cand"] < NFs for b in HIT_FRAMES), name
        assert set(c["planted"][0]) >= {i for i in (0, 255, 256, 257, 511, 512, NFs - 1) if i < NFs}
        for b in HIT_FRAMES:
            v = full[b]["v"][full[b]["collide"]]; gate = M.value_gate(full[b], C.E32["order"][0])
            for mc in C.ORDER_MAX_COLL:
                k = min(mc, len(v)); sums = np.sort([v[list(s)].sum() for s in itertools.combinations(range(len(v)), k)])
                if len(sums) > 1:
                    least = min(least, float(np.diff(sums).min() / gate)); assert np.diff(sums).min() > 100 * gate, (name, b, mc)
                kept = C.reference(name, mc)[b]; assert list(kept["kept"][:, 1]) == c["planted"][b][:k]
    assert seen >= {0, 254, 255, 256, 257, 510, 511, 512, 699}
    print("order: the closest two subsets of one size are %.0f value gates apart (at least 100 asked)" % least)


def test_block_case_shapes():
    for name, _ in C.FAMILY["blocks"]:
        c = C.case(name); NFo, NVo = len(c["of"]), c["ov"].shape[1]; ref = C.reference(name)
        assert (NFo, NVo) in C.BLOCKS and len(c["sf"]) == 312 and len(c["sv"]) == 3 and all(r["pairs"] > 0 for r in ref)
        assert C.search_block_seed(NFo, NVo) == c["seed"]
        with_pairs = set(np.concatenate([r["kept"][:, 0] for r in ref]).tolist())          # every face at a block edge has a kept pair in some frame
        edge = C.block_edge_faces(NFo); assert set(edge) <= with_pairs and {0, NFo - 1} <= set(edge) and {i for i in (254, 255, 256, 511, 512) if i < NFo} <= set(edge), (name, edge)
        if NFo > 1:                                       # the last vertex belongs to one face; without it in the object's box a kept pair is lost in some frame
            assert (c["of"] == NVo - 1).sum() == 1 and not (c["of"][edge] == NVo - 1).any(); lost = 0
            for b, r in enumerate(ref):
                blo, bhi = c["ov"][b][:-1].min(0), c["ov"][b][:-1].max(0); S = c["sv"][b][c["sf"]][r["kept"][:, 1]]
                lost += int((~((S.min(1) <= bhi).all(1) & (blo <= S.max(1)).all(1))).sum())
            assert lost > 0, name


def test_float32_oracle_takes_the_models_decisions_and_E32_is_current():
    for fam, cases in C.FAMILY.items():
        eV = eg = 0.0
        for name, mc in cases:
            a, b, differ = C.measure_e32(name, mc); eV, eg = max(eV, a), max(eg, b)
            assert differ == 0, (name, mc, differ)
        print("E32[%s]: measured value %.4f, gradient %.4f (u S); recorded %s" % (fam, eV, eg, C.E32[fam]))
        for rec, got in zip(C.E32[fam], (eV, eg)):
            assert got / 2 <= rec <= 2 * got, (fam, rec, got)


# ---- the product's header on the host ----------------------------------------------------------------------------------------------------------------------------
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "collide_geom.h"
/* in: int32 B NVs NFs NVo NFo max_coll, float sigma, sv (B NVs 3) float, sf (NFs 3) int32, ov (B NVo 3) float, of (NFo 3) int32.  out: per frame 5 doubles: value, d/dt xyz, pairs.
   The pairs are walked the way collide.hip walks them: object box, SMPL faces overlapping it in face order, per object face the first max_coll that collide. */
static void tri(const float *v, const int *f, float *T) { for (int c = 0; c < 3; c++) for (int k = 0; k < 3; k++) T[3 * c + k] = v[3 * (size_t)f[c] + k]; }
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"); if (!in) return 3;
    int h[6]; float sigma;
    if (fread(h, 4, 6, in) != 6 || fread(&sigma, 4, 1, in) != 1) return 4;
    const int B = h[0], NVs = h[1], NFs = h[2], NVo = h[3], NFo = h[4], mc = h[5];
    float *sv = malloc(sizeof(float) * 3 * B * NVs), *ov = malloc(sizeof(float) * 3 * B * NVo);
    int *sf = malloc(sizeof(int) * 3 * NFs), *of = malloc(sizeof(int) * 3 * NFo), *cand = malloc(sizeof(int) * NFs);
    if (fread(sv, 4, (size_t)3 * B * NVs, in) != (size_t)3 * B * NVs || fread(sf, 4, (size_t)3 * NFs, in) != (size_t)3 * NFs) return 4;
    if (fread(ov, 4, (size_t)3 * B * NVo, in) != (size_t)3 * B * NVo || fread(of, 4, (size_t)3 * NFo, in) != (size_t)3 * NFo) return 4;
    fclose(in);
    FILE *out = fopen(argv[2], "wb"); if (!out) return 5;
    for (int b = 0; b < B; b++) {
        const float *vs = sv + (size_t)3 * b * NVs, *vo = ov + (size_t)3 * b * NVo;
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int i = 0; i < NVo; i++) for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], vo[3 * i + k]); hi[k] = fmaxf(hi[k], vo[3 * i + k]); }
        int n = 0;
        for (int f = 0; f < NFs; f++) { float T[9], tlo[3], thi[3]; tri(vs, sf + 3 * f, T); col_tri_box(T, tlo, thi); if (col_box_overlap(tlo, thi, lo, hi)) cand[n++] = f; }
        double r[5] = {0, 0, 0, 0, 0};
        for (int fo = 0; fo < NFo; fo++) {
            float To[9], olo[3], ohi[3]; tri(vo, of + 3 * fo, To); col_tri_box(To, olo, ohi);
            int found = 0;
            for (int i = 0; i < n && found < mc; i++) {
                float Ts[9], slo[3], shi[3], gd[3]; tri(vs, sf + 3 * cand[i], Ts); col_tri_box(Ts, slo, shi);
                if (!col_box_overlap(slo, shi, olo, ohi) || !col_tri_tri(To, Ts)) continue;
                found++;
                r[0] += (double)col_pair_side(Ts, To, sigma, gd); for (int k = 0; k < 3; k++) r[1 + k] += gd[k];
                r[0] += (double)col_pair_side(To, Ts, sigma, gd); for (int k = 0; k < 3; k++) r[1 + k] -= gd[k];
            }
            r[4] += found;
        }
        fwrite(r, 8, 5, out);
    }
    fclose(out);
    return 0;
}
"""


@pytest.fixture(scope="module")
def header_driver(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    d = tmp_path_factory.mktemp("collide_host"); src = d / "driver.c"; src.write_text(DRIVER); exe = d / "driver"
    subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "vistracker_amd", "csrc"), "-o", str(exe), str(src), "-lm"])

    def run(name, max_coll):
        c = C.case(name); B = len(c["sv"]); f = d / "case.bin"
        with open(f, "wb") as fh:
            fh.write(np.array([B, c["sv"].shape[1], len(c["sf"]), c["ov"].shape[1], len(c["of"]), max_coll], np.int32).tobytes()); fh.write(np.float32(c["sigma"]).tobytes())
            for a in (c["sv"], c["sf"], c["ov"], c["of"]):
                fh.write(np.ascontiguousarray(a).tobytes())
        subprocess.check_call([str(exe), str(f), str(d / "out.bin")])
        return np.fromfile(d / "out.bin", np.float64).reshape(B, 5)
    return run


@pytest.mark.parametrize("family", list(C.FAMILY))
def test_the_products_header_meets_the_gates_on_the_host(header_driver, family):
    """collide_geom.h in float32 on the CPU, pairs walked like the kernels: counts equal to the model's on decided frames, value and gradient inside the GPU test's
    gates (without the fixed-point term they are only tighter here by n_f 2^-41)"""
    wV = wg = 0.0; EV, Eg = C.E32[family]
    for name, mc in C.FAMILY[family]:
        out = header_driver(name, mc)
        for b, r in enumerate(C.reference(name, mc)):
            if r["undecided"].any():
                assert family in ("pairs", "fit_like")
                match = [q for q in M.resolutions(r, mc) if q["pairs"] == int(out[b, 4]) and abs(out[b, 0] - q["V"]) <= M.value_gate(q, EV)
                         and (np.abs(out[b, 1:4] - q["g"]) <= M.grad_gate(q, Eg, 1.0, 1)).all()]
                assert match, (name, b, "no resolution of the undecided pairs gives the header's result")
                continue
            assert int(out[b, 4]) == r["pairs"], (name, mc, b, out[b, 4], r["pairs"])
            fV = abs(out[b, 0] - r["V"]) / M.value_gate(r, EV) if r["pairs"] else float(out[b, 0] != 0)
            fg = float((np.abs(out[b, 1:4] - r["g"]) / M.grad_gate(r, Eg, 1.0, 1)).max()) if r["pairs"] else float(out[b, 1:4].any())
            wV, wg = max(wV, fV), max(wg, fg)
            assert fV <= 1 and fg <= 1, (name, mc, b, fV, fg)
    print("collide_geom.h on the host, %s: worst value error %.3f of its gate, worst gradient error %.3f of its gate" % (family, wV, wg))
