"""Worker of tests/test_gpu_step_gemm_forms.py: a fresh process, started with PMK_STEP_GEMM set, fits every case of
CASES and writes L, c, the -D^-1 blocks and info of every patch into one .npz (argv[1])."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# n with nt = 2, 3 and 5 tiles and a ragged last tile; 296 = 2 * 128 + 40: the last block row has waves (rows 64 ..)
# entirely in the padding; 328 = 2 * 128 + 72: its third wave is partly padding
TILE_SIZES = [129, 300, 640 - 7, 2 * 128 + 40, 2 * 128 + 72]
# 11 patches (the dealing over 8 XCDs has a remainder), nt = 2, 3 and 5 mixed: the end-aligned schedule starts the small
# patches at later launches
RAGGED = [633, 129, 300, 296, 328, 520, 257, 640, 200, 385, 131]
# name -> (sizes, D, dtype, bad): `bad` = (patch, row) whose diagonal gets -10 (not positive definite from that pivot)
CASES = {}
for _dt in ("f64", "f32"):
    for _n in TILE_SIZES:
        CASES["tiles-%d-%s" % (_n, _dt)] = ([_n], 2, _dt, None)
    for _D in (1, 2, 3):                         # D = 2, 3: fused evaluation of the tiles; D = 1: tiles loaded
        CASES["ragged-D%d-%s" % (_D, _dt)] = (RAGGED, _D, _dt, None)
    CASES["notpd-%s" % _dt] = ([300, 633, 296, 129, 520], 2, _dt, (1, 400))


def case_data(name):
    sizes, D, dtype, bad = CASES[name]
    rng = np.random.Generator(np.random.PCG64(sum(map(ord, name))))
    Xs = [rng.uniform(-4, 4, (n, D)) for n in sizes]
    ys = [np.sin(x[:, 0]) * np.cos(0.5 * x[:, -1]) for x in Xs]
    return sizes, D, dtype, bad, Xs, ys


def main():
    import patchmixturekriging_amd as pmk
    from patchmixturekriging_amd import mixture as M
    th = pmk.Spline34KernelType(1 / 3.0)
    out = {}
    for name in CASES:
        sizes, D, dtype, bad, Xs, ys = case_data(name)
        model = M.DeviceModel(Xs, ys, dtype=dtype)
        if bad is not None:
            ds = [np.zeros(n) for n in sizes]
            ds[bad[0]][bad[1]] = -10.0
            model.set_diag(ds)
        model.fit(th, 5e-2)
        out[name + "/info"] = model.info()
        for r in range(len(sizes)):
            out["%s/%d/L" % (name, r)] = model.get(r, M.GET_L)
            out["%s/%d/c" % (name, r)] = model.get(r, M.GET_C)
            out["%s/%d/ninv" % (name, r)] = model.get(r, M.GET_LINV_DIAG)
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
