"""The host's tile-choice rules (physicsvae_amd/csrc/pvae_gemm_launch.h), restated: the selectors, make_grid, the planner of
the forward / input-gradient family (tile_geometry + plan_tiles) and plan_wgrad.  Whoever retunes a selector learns from
the tests that import this (test_fc_cases_cpu.py, test_tile_plan_cpu.py) that the sweeps must follow."""

OPTIONS = {"ws64": 1, "ws6464": 1, "ws6464_rows": 1, "pair64": 1, "dgrad16": 1, "wgrad32": 1, "krot": 0, "rowxcd": 0}


def forward_uses_16x16(m, n):                                    # forward_uses_16x16
    return (m // 32) * (n // 32) < 128


def dgrad_uses_16x16(m, k_in, dgrad16=1):                        # dgrad_uses_16x16 (option "dgrad16")
    return bool(dgrad16) and (m // 32) * (k_in // 32) < 128


def wgrad_uses_32x32(n, k_in, m, wgrad32=1):                     # wgrad_uses_32x32 (option "wgrad32": 0 never, 2 always)
    return bool(wgrad32) and ((n // 64) * (k_in // 64) <= 128 or wgrad32 == 2) and m % 64 == 0


def uses_64x32(m, n, ws64=1):                                    # uses_64x32 (option "ws64")
    return bool(ws64) and m >= 512 and m % 64 == 0 and (m // 64) * (n // 32) >= 256


def uses_64x64(m, n, ws64=1, ws6464=1):                          # uses_64x64 (option "ws6464")
    return bool(ws6464) and uses_64x32(m, n, ws64) and n % 64 == 0 and (m // 64) * (n // 64) >= 256


def make_grid(rows_q, cols_p, bq, bp):                           # make_grid: every XCD a contiguous range of p-tiles
    tiles_q, tiles_p = rows_q // bq, cols_p // bp
    p_per_xcd = (tiles_p + 7) // 8
    return tiles_q, tiles_p, p_per_xcd, 8 * p_per_xcd * tiles_q


# what a call site opens (TileRule): wide geometries, 64x32 alone for a pair, the 16x16 rule, krot / rowxcd held at 0
RULES = {
    "forward": (True, False, "forward", False),                  # gemm_forward_epi<EpiBiasAct>
    "forward_epi": (False, False, "forward", False),             # gemm_forward_epi<another epilogue>, forward_tiles
    "gather": (True, False, None, False),                        # gemm_forward_gather<EpiBiasAct>
    "gather_epi": (False, False, None, False),
    "dgrad": (True, False, "dgrad", False),                      # gemm_dgrad_epi<EpiMask>
    "dgrad_epi": (False, False, "dgrad", False),                 # gemm_dgrad_epi<another epilogue>, plan_dgrad, dgrad_tiles
    "pair": (False, True, "dgrad", False),                       # gemm_bwd_pair_epi<EpiMask, .>
    "fc_forward": (False, False, "forward", True),               # pvae_fc.hip fwd_prob
    "fc_dgrad": (False, False, "dgrad", True),                   # pvae_fc.hip d_prob
}
TILE = {"16x16": (16, 16), "32x32": (32, 32), "64x32": (64, 32), "64x64": (64, 64)}


def ga_flags(krot, tile32, tile16, rowxcd):
    return (krot & 7) | (int(tile32) << 3) | (int(tile16) << 4) | ((rowxcd & 1) << 5)


def plan_tiles(rule, m, n, **options):
    """(geometry, tiles_q, tiles_p, p_per_xcd, grid, flag bits) of an [m x n] output."""
    o = dict(OPTIONS, **options)
    wide, pair, narrow, plain = RULES[rule]
    w32 = uses_64x32(m, n, o["ws64"])
    if wide and uses_64x64(m, n, o["ws64"], o["ws6464"]):
        geom = "64x64"
    elif (wide and w32) or (pair and o["pair64"] and w32):
        geom = "64x32"
    elif (narrow == "forward" and forward_uses_16x16(m, n)) or (narrow == "dgrad" and dgrad_uses_16x16(m, n, o["dgrad16"])):
        geom = "16x16"
    else:
        geom = "32x32"
    tiles_q, tiles_p, p_per_xcd, grid = make_grid(m, n, *TILE[geom])
    krot, rowxcd = (0, 0) if plain else (o["krot"], o["rowxcd"])
    if geom == "64x64" and o["ws6464_rows"]:                     # the XCDs partition the row blocks
        rowxcd, grid = 1, 8 * ((tiles_q + 7) // 8) * tiles_p
    return geom, tiles_q, tiles_p, p_per_xcd, grid, ga_flags(krot, 0, geom == "16x16" and narrow == "dgrad", rowxcd)


def plan_wgrad(n, k_in, m, plain=False, **options):
    """(tile32, tiles_q, tiles_p, p_per_xcd, grid, bias workgroups, flag bits) of the [n x k_in] weight gradient over m rows."""
    o = dict(OPTIONS, **options)
    t32 = wgrad_uses_32x32(n, k_in, m, o["wgrad32"])
    tiles_q, tiles_p, p_per_xcd, grid = make_grid(n, k_in, *((32, 32) if t32 else (64, 64)))
    krot, rowxcd = (0, 0) if plain else (o["krot"], o["rowxcd"])
    return int(t32), tiles_q, tiles_p, p_per_xcd, grid, n // 32, ga_flags(krot, t32, 0, rowxcd)
