"""The geometries of tests/test_conv_pipe_balanced_gpu.py, (N, H, W, Cin, Cout, k, s, p) as in
tests/exact_conv.py, with the tile and K-step counts the balanced schedule sees on cfg 90
(256-pixel x 256-channel tiles, 64-deep K steps).  tests/test_conv_pipe_plan_cpu.py asserts on
the CPU that integer operands keep every result of these shapes exact."""

FWD = (20, 8, 8, 256, 256, 3, 1, 1)     # 5 tiles, S = 36: G = 4 splits tiles 1, 2 and 3
L4 = (16, 7, 7, 512, 512, 3, 1, 1)      # 4 M tiles (the last with 16 rows) x 2 N tiles, S = 72
ALIGNED = (16, 8, 8, 256, 256, 3, 1, 1)  # 4 tiles, G = 2: ranges end on tile boundaries
ONE_TAP = (20, 8, 8, 256, 256, 1, 1, 0)  # S = C / 64 = 4
STRIDE2 = (8, 16, 16, 256, 256, 3, 2, 1)  # four parity classes (and the merged projection)
ALL = [FWD, L4, ALIGNED, ONE_TAP, STRIDE2]


def tiles_steps(geom, dgrad):
    """(T, S) of the cfg-90 launch of a stride-1 geometry: forward, or its data gradient."""
    N, H, W, Cin, Cout, k, s, p = geom
    assert s == 1
    OH, OW = (H + 2 * p - k) + 1, (W + 2 * p - k) + 1
    M, C, ncols = (N * H * W, Cout, Cin) if dgrad else (N * OH * OW, Cin, Cout)
    return (M + 255) // 256 * (ncols // 256), k * k * C // 64
