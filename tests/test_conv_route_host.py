"""The routing table of ydbl_conv2d_nhwc, pinned through ydbl_conv_route (include/ydbl.h): kernel family, template
instance, split, epilogue form and grid of the real threshold shapes, under the default switches and under each
YDBL_* switch.  No GPU: the descriptors carry fake device pointers and nothing is launched.

Every expected record was worked out by hand from the routing rules as they stood before conv_route.hpp gathered
them (the arithmetic is in the comments), not read back from the function under test."""

import pytest

SWITCHES = ("YDBL_SPLITK", "YDBL_HALO_NB", "YDBL_HALO_SMALL", "YDBL_VW", "YDBL_WSK_HALF", "YDBL_EPI_GENERIC")
VW, TILE, HALO, WSK, IGEMM = range(5)
SILU, RT, ANY = 1, -1, -2  # epi: compiled SiLU, the runtime form, the kernel's own per-wave choice
PTR = 0x7F0000001000  # fake, 16-byte aligned


def _desc(cin, cout, k, s, n, h, w, dtype="f16", fp8=False, ws=False):
    """A valid descriptor of a k x k / stride s / pad k // 2 conv with SiLU.  ws: it carries the workspace
    ydbl_conv_workspace asks for, as the plan builder gives it."""
    from ydbl import _lib

    dt = _lib.F16 if dtype == "f16" else _lib.F32
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    d = _lib.ConvDesc()
    d.x = _lib.View(PTR, n, h, w, cin, cin, dt)
    d.y = _lib.View(PTR + (1 << 32), n, ho, wo, cout, cout, dt)
    d.w, d.bias = PTR + (2 << 32), PTR + (3 << 32)
    d.kh = d.kw = k
    d.stride, d.pad, d.dil = s, k // 2, 1
    d.kpad = (k * k * cin + 31) // 32 * 32
    d.act, d.res_mode = _lib.ACT_SILU, _lib.RES_NONE
    if fp8:
        d.dq, d.qscale = PTR + (4 << 32), 1.0
    if ws:
        d.workspace, d.workspace_bytes = PTR + (5 << 32), _lib.lib.ydbl_conv_workspace(d)
    return d


def _route(d):
    from ydbl import _lib

    r = _lib.ConvRouteInfo()
    assert _lib.lib.ydbl_conv_route(d, r) == 0, _lib.lib.ydbl_last_error()
    assert _lib.lib.ydbl_conv_workspace(d) == r.workspace_bytes  # one function answers both queries
    return (r.family, list(r.v), r.pointwise, r.ksplit, r.epi, list(r.grid), r.workspace_bytes)


# name: (descriptor arguments, environment, expected (family, v, pointwise, ksplit, epi, grid, workspace bytes))
# P = output pixels, K = k * k * Cin; tiles: the halo / VGPR-weight kernels' 8 x 16, ceil(Ho / 8) * ceil(Wo / 16)
CASES = {
    # thin input, 80^2 >= 4096 pixels per image: Cin 16, (32 + 15) / 16 = 2 channel tiles, stride 1 -> 8 x 32 tiles,
    # 2 * 10 * 3 workgroups; fp16 SiLU, Cout % 4 == 0, one output: the epilogue compiled as SiLU
    "tile": ((16, 32, 3, 1, 2, 80, 80), {}, (TILE, [16, 2, 1, 0], 0, 1, SILU, [60, 1, 1], 0)),
    # P = 25600 (not below): halo; two images per workgroup, 32-channel slices: 8 * 15 tiles * 2 slices
    "halo-nblock": ((384, 64, 3, 1, 16, 40, 40), {}, (HALO, [1, 2, 32, 0], 0, 1, ANY, [240, 1, 1], 0)),
    # one image per workgroup: 240 tiles * 1 64-channel slice < 512 -> 32-channel slices, 240 * 2
    "halo-nb1": ((384, 64, 3, 1, 16, 40, 40), {"YDBL_HALO_NB": "1"}, (HALO, [1, 1, 32, 0], 0, 1, ANY, [480, 1, 1], 0)),
    # P = 6400 < 25600, 24 chunks >= 8, 60 tiles * 4 slices = 240 workgroups -> min(4, ceil(512 / 240)) = 3 splits of
    # 8 chunks; partials 3 * 6400 * 128 * 4 bytes
    "halo-splitk": ((768, 128, 3, 1, 4, 40, 40, "f16", False, True), {},
                    (HALO, [1, 1, 32, 0], 0, 3, ANY, [240, 3, 1], 9830400)),
    # no room: not the halo kernel (splittable, so not its small-map form either) -> wave-split-K, K = 6912;
    # Cout 128 and ceil(6400 / 32) * 1 = 200 < 256 workgroups -> 32 x 64 tiles, 200 x 2 = 400 < 768 tiles, 54 steps ->
    # min(4, ceil(768 / 400)) = 2 splits, no room for them either -> unsplit
    "halo-splitk-no-workspace": ((768, 128, 3, 1, 4, 40, 40), {},
                                 (WSK, [32, 64, 0, 0], 0, 1, ANY, [200, 2, 1], 9830400)),
    # no split -> the small-map halo tile (Cout >= 128): two images per workgroup, 2 * 15 tiles * 4 slices
    "halo-splitk-off": ((768, 128, 3, 1, 4, 40, 40, "f16", False, True), {"YDBL_SPLITK": "0"},
                        (HALO, [1, 2, 32, 0], 0, 1, ANY, [120, 1, 1], 0)),
    # P = 1600 < 4096: not the halo kernel; 50 < 256 workgroups -> 32 x 64 tiles, 100 tiles, 54 steps ->
    # min(4, ceil(768 / 100)) = 4 splits of 13 steps; partials 4 * 1600 * 128 * 4 bytes
    "wsk-splitk": ((768, 128, 3, 1, 4, 20, 20, "f16", False, True), {},
                   (WSK, [32, 64, 0, 0], 0, 4, ANY, [50, 2, 4], 3276800)),
    # no half-height tiles: Cout % 128 == 0 -> 32 x 128, 50 tiles -> 4 splits
    "wsk-half-off": ((768, 128, 3, 1, 4, 20, 20, "f16", False, True), {"YDBL_WSK_HALF": "0"},
                     (WSK, [32, 128, 0, 0], 0, 4, ANY, [50, 1, 4], 3276800)),
    # P = 6400, 4 chunks < 8: unsplittable, Cout 256 >= 128 -> the small-map halo tile, 2 * 15 tiles * 8 slices
    "halo-small": ((128, 256, 3, 1, 4, 40, 40), {}, (HALO, [1, 2, 32, 0], 0, 1, ANY, [240, 1, 1], 0)),
    # -> wave-split-K, K = 1152: Cout > 128 -> 32 x 128 (Cout % 128 == 0), 200 x 2 tiles, 9 steps < 16: unsplit
    "halo-small-off": ((128, 256, 3, 1, 4, 40, 40), {"YDBL_HALO_SMALL": "0"},
                       (WSK, [32, 128, 0, 0], 0, 1, ANY, [200, 2, 1], 0)),
    # 64 -> 64 with 25601 <= P = 51200 <= 65536: the Cin-64 instance, 8-row tiles, 8 * 10 * 5 workgroups
    "vw-64": ((64, 64, 3, 1, 8, 80, 80), {"YDBL_VW": "1"}, (VW, [64, 8, 0, 0], 0, 1, ANY, [400, 1, 1], 0)),
    # default: halo (P >= 25600), two images per workgroup: 4 * 50 tiles * 2 slices
    "vw-64-off": ((64, 64, 3, 1, 8, 80, 80), {}, (HALO, [1, 2, 32, 0], 0, 1, ANY, [400, 1, 1], 0)),
    # 128 -> 64 at any size: the Cin-128 instance, 16 * 5 * 3 workgroups
    "vw-128": ((128, 64, 3, 1, 16, 40, 40), {"YDBL_VW": "1"}, (VW, [128, 8, 0, 0], 0, 1, ANY, [240, 1, 1], 0)),
    "vw-128-off": ((128, 64, 3, 1, 16, 40, 40), {}, (HALO, [1, 2, 32, 0], 0, 1, ANY, [240, 1, 1], 0)),
    # stride 2, P = 204800 (not below): halo stride 2, one image per workgroup; 8 * 20 * 10 = 1600 tiles * 4 64-channel
    # slices >= 512 -> 64-channel slices
    "halo-s2": ((128, 256, 3, 2, 8, 320, 320), {}, (HALO, [2, 1, 64, 0], 0, 1, ANY, [6400, 1, 1], 0)),
    # P = 179200 < 204800: not the halo kernel; K = 1152 >= 1024 -> wave-split-K (the block GEMM takes the stride-2
    # convs below the threshold only where K < 1024: the next pair), 32 x 128 tiles: 5600 x 2 >= 768, unsplit
    "halo-s2-below": ((128, 256, 3, 2, 7, 320, 320), {}, (WSK, [32, 128, 0, 0], 0, 1, ANY, [5600, 2, 1], 0)),
    # K = 576 < 1024 (and P > 16384): P = 204800 -> halo stride 2, 1600 tiles * 2 64-channel slices
    "halo-s2-k576": ((64, 128, 3, 2, 8, 320, 320), {}, (HALO, [2, 1, 64, 0], 0, 1, ANY, [3200, 1, 1], 0)),
    # P = 179200: block GEMM; want 1024 workgroups (Cout <= 128 but P > 65536, K > 128): 1400 x 2 of 128 x 64 do;
    # not pointwise: the runtime epilogue form
    "igemm-s2-below": ((64, 128, 3, 2, 7, 320, 320), {}, (IGEMM, [128, 64, 2, 2], 0, 1, RT, [1400, 2, 1], 0)),
    # 1x1, K = 512 but P = 51200 > 16384: block GEMM; Cout <= 128 and P <= 65536 -> want 512: 400 x 2 of 128 x 64 do;
    # pointwise fp16 SiLU: compiled as SiLU
    "igemm-1x1": ((512, 128, 1, 1, 32, 40, 40), {}, (IGEMM, [128, 64, 2, 2], 1, 1, SILU, [400, 2, 1], 0)),
    "igemm-1x1-generic": ((512, 128, 1, 1, 32, 40, 40), {"YDBL_EPI_GENERIC": "1"},
                          (IGEMM, [128, 64, 2, 2], 1, 1, RT, [400, 2, 1], 0)),
    # 1x1, K = 2048: wave-split-K 32 x 128 (Cout % 128 == 0), 50 x 2 tiles, 16 steps -> min(4, 8) splits, each
    # >= 8 steps: 2; partials 2 * 1600 * 256 * 4 bytes
    "wsk-1x1-splitk": ((2048, 256, 1, 1, 4, 20, 20, "f16", False, True), {},
                       (WSK, [32, 128, 0, 0], 1, 2, ANY, [50, 2, 2], 3276800)),
    # fp32 never splits (one summation order): "wsk-splitk" in fp32 asks for no workspace and runs unsplit
    "wsk-f32": ((768, 128, 3, 1, 4, 20, 20, "f32", False, True), {}, (WSK, [32, 64, 0, 0], 0, 1, ANY, [50, 2, 1], 0)),
    # fp8 operands skip the thin-input tile ("tile" above): block GEMM, want 512, Cout <= 32: 50 / 100 workgroups of
    # 256 / 128 x 32 are too few -> 64 x 32, 200; the runtime epilogue form
    "fp8-not-tile": ((16, 32, 3, 1, 2, 80, 80, "f16", True), {}, (IGEMM, [64, 32, 4, 1], 0, 1, RT, [200, 1, 1], 0)),
    # ... and the VGPR-weight kernel ("vw-64"): halo, one image per workgroup (no fp8 N-blocking), 400 tiles < 512 ->
    # 32-channel slices
    "fp8-not-vw": ((64, 64, 3, 1, 8, 80, 80, "f16", True), {"YDBL_VW": "1"},
                   (HALO, [1, 1, 32, 0], 0, 1, ANY, [800, 1, 1], 0)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_conv_route(name, monkeypatch):
    args, env, want = CASES[name]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert _route(_desc(*args)) == want


def test_conv_route_reads_the_switches_per_call(monkeypatch):
    """One process, one descriptor: each switch moves the route as soon as it is set."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    d = _desc(384, 64, 3, 1, 16, 40, 40)
    base = _route(d)
    monkeypatch.setenv("YDBL_HALO_NB", "2")  # only '1' is "off"
    assert _route(d) == base
    monkeypatch.setenv("YDBL_HALO_NB", "1")
    assert _route(d) != base
    monkeypatch.delenv("YDBL_HALO_NB")
    assert _route(d) == base


def test_conv_route_rejects_bad_arguments():
    from ydbl import _lib

    assert _lib.lib.ydbl_conv_route(None, _lib.ConvRouteInfo()) == 1
    assert _lib.lib.ydbl_conv_route(_desc(16, 32, 3, 1, 2, 80, 80), None) == 1
    d = _desc(16, 32, 3, 1, 2, 80, 80)
    d.kpad = 100
    assert _lib.lib.ydbl_conv_route(d, _lib.ConvRouteInfo()) == 1 and _lib.lib.ydbl_conv_workspace(d) == -1
