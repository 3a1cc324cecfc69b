"""The host's tile planner (pvae_gemm_launch.h: tile_geometry / plan_tiles, plan_wgrad) against the restatement of
tests/tile_rules.py, without a GPU: a stand-alone HOST program includes the launch header, sets the option globals and
prints every plan of a sweep -- geometry, tile counts, p-tiles per XCD, grid, flag bits -- for every kind of call site.
The sweep holds both sides of every boundary of the selectors; it runs at the default options and with each option moved."""
import os
import shutil
import subprocess

import pytest

import tile_rules as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

# [M x N] outputs of the forward / input-gradient family
SHAPES = [
    (32, 32), (64, 64), (256, 256), (256, 1024),
    (128, 992), (128, 1024),             # (M/32)(N/32) = 124 | 128: 16x16 | 32x32
    (512, 992), (512, 1024),             # (M/64)(N/32) = 248 | 256: 32x32 | 64x32
    (544, 1024), (480, 2048),            # >= 512 rows that are no multiple of 64; under 512 rows
    (1024, 960), (1024, 1024),           # (M/64)(N/64) = 240 | 256: 64x32 | 64x64
    (1024, 1056),                        # N % 64 != 0 at 1024 rows: 64x32
    (2048, 1024), (2048, 64), (2048, 96), (1088, 1024),     # row blocks that are no multiple of the 8 XCDs: 17
]
# weight gradients [N x Kin] over M rows
WSHAPES = [
    (1024, 512, 256), (1024, 576, 256), (640, 832, 256),    # (N/64)(Kin/64) = 128 | 144, 130: 32x32 | 64x64
    (1024, 520, 256),                                       # (Kin / 64 rounds down: 128 still)
    (1024, 512, 96), (64, 64, 32), (64, 64, 64),            # M % 64 != 0: 64x64 whatever the size
    (1024, 1024, 1024), (256, 64, 2048),
]
OPTION_RUNS = [{}] + [{k: 0} for k in ("ws64", "ws6464", "ws6464_rows", "pair64", "dgrad16", "wgrad32")] + [
    {"wgrad32": 2}, {"krot": 1, "rowxcd": 1}]

PROGRAM = r"""
#include "pvae_gemm_launch.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace pvae;
int main(int argc, char** argv) {
    struct { const char* name; int* v; } opts[] = {{"ws64", &g_ws64}, {"ws6464", &g_ws6464}, {"ws6464_rows", &g_ws6464_rows},
        {"pair64", &g_pair64}, {"dgrad16", &g_dgrad16}, {"wgrad32", &g_wgrad32}, {"krot", &g_krot}, {"rowxcd", &g_rowxcd}};
    struct { const char* name; TileRule r; } rules[] = {
        {"forward", {true, false, TileRule::kForward, false}}, {"forward_epi", {false, false, TileRule::kForward, false}},
        {"gather", {true, false, TileRule::kNever, false}}, {"gather_epi", {false, false, TileRule::kNever, false}},
        {"dgrad", {true, false, TileRule::kDgrad, false}}, {"dgrad_epi", {false, false, TileRule::kDgrad, false}},
        {"pair", {false, true, TileRule::kDgrad, false}}, {"fc_forward", {false, false, TileRule::kForward, true}},
        {"fc_dgrad", {false, false, TileRule::kDgrad, true}}};
    const char* geom[] = {"16x16", "32x32", "64x32", "64x64"};
    for (int i = 1; i < argc; ++i) {
        int a, b, c;
        char name[32];
        if (sscanf(argv[i], "%31[a-z0-9_]=%d", name, &a) == 2) {
            bool known = false;
            for (auto& o : opts) if (!strcmp(o.name, name)) { *o.v = a; known = true; }
            if (!known) return 2;
        } else if (sscanf(argv[i], "t:%dx%d", &a, &b) == 2) {
            for (auto& r : rules) {
                const TilePlan t = plan_tiles(r.r, nullptr, 0, nullptr, 0, a, b, 64);
                printf("%s %d %d %s %d %d %d %d %d\n", r.name, a, b, geom[t.geom], t.ga.tiles_q, t.ga.tiles_p, t.ga.p_per_xcd, t.grid,
                       ga_flags(t.ga));
            }
            if (forward_tiles(a, b) != plan_tiles(rules[1].r, nullptr, 0, nullptr, 0, a, b, 0).tiles()) return 3;
            if (dgrad_tiles(a, b) != plan_dgrad(nullptr, 0, nullptr, 0, a, b, 0).tiles()) return 3;
        } else if (sscanf(argv[i], "w:%dx%dx%d", &a, &b, &c) == 3) {
            for (int plain = 0; plain < 2; ++plain) {
                const WgradPlan w = plan_wgrad(nullptr, 0, nullptr, 0, a, b, c, plain != 0);
                printf("%s %d %d %d %d %d %d %d %d %d %d\n", plain ? "fc_wgrad" : "wgrad", a, b, c, w.ga.tile32, w.ga.tiles_q, w.ga.tiles_p,
                       w.ga.p_per_xcd, w.grid, w.nbias, ga_flags(w.ga));
            }
        } else
            return 2;
    }
    return 0;
}
"""


def expected(options):
    lines = []
    for m, n in SHAPES:
        for rule in T.RULES:
            lines.append("%s %d %d %s %d %d %d %d %d" % ((rule, m, n) + T.plan_tiles(rule, m, n, **options)))
    for n, k_in, m in WSHAPES:
        for plain in (False, True):
            lines.append("%s %d %d %d %d %d %d %d %d %d %d" % (("fc_wgrad" if plain else "wgrad", n, k_in, m) +
                                                                T.plan_wgrad(n, k_in, m, plain, **options)))
    return lines


def test_the_sweep_holds_both_sides_of_every_boundary():
    geoms = {rule: {T.plan_tiles(rule, m, n)[0] for m, n in SHAPES} for rule in T.RULES}
    assert geoms["forward"] == geoms["dgrad"] == {"16x16", "32x32", "64x32", "64x64"}
    assert geoms["gather"] == {"32x32", "64x32", "64x64"} and geoms["pair"] == {"16x16", "32x32", "64x32"}
    assert geoms["forward_epi"] == geoms["dgrad_epi"] == geoms["fc_forward"] == geoms["fc_dgrad"] == {"16x16", "32x32"}
    assert [(m // 32) * (n // 32) for m, n in SHAPES[4:6]] == [124, 128]
    assert [(m // 64) * (n // 32) for m, n in SHAPES[6:8]] == [248, 256]
    assert [(m // 64) * (n // 64) for m, n in SHAPES[10:12]] == [240, 256]
    assert any(m >= 512 and m % 64 for m, n in SHAPES) and any(m == 2048 for m, n in SHAPES)
    assert any(m == 1024 and n % 64 and T.uses_64x32(m, n) for m, n in SHAPES)
    assert any((m // 64) % 8 and T.uses_64x64(m, n) for m, n in SHAPES)          # the row-XCD grid rounds up
    assert [(n // 64) * (k // 64) for n, k, m in WSHAPES[:4]] == [128, 144, 130, 128]
    assert {T.plan_wgrad(*s)[0] for s in WSHAPES} == {0, 1} and any(m % 64 for n, k, m in WSHAPES)
    # the wide classes and the 16x16 classes are disjoint (what makes the planner's order of checks immaterial)
    for m in range(32, 2049, 32):
        for n in range(32, 2049, 32):
            assert not (T.uses_64x32(m, n) and (T.forward_uses_16x16(m, n) or T.dgrad_uses_16x16(m, n)))


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_planner_matches_the_restated_rules(tmp_path):
    src = tmp_path / "tile_plan.hip"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "tile_plan")
    r = subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-I",
                        os.path.join(ROOT, "physicsvae_amd", "csrc"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    shapes = ["t:%dx%d" % s for s in SHAPES] + ["w:%dx%dx%d" % s for s in WSHAPES]
    for options in OPTION_RUNS:
        r = subprocess.run([exe] + ["%s=%d" % kv for kv in options.items()] + shapes, capture_output=True, text=True)
        assert r.returncode == 0, (options, r.returncode, r.stderr[-2000:])
        got, want = r.stdout.split("\n")[:-1], expected(options)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g == w, (options, g, w)
