"""Print fdm_gemm_heuristic_tile over a grid of shapes, operand kinds and launch forms, one line per point (host only: no GPU).
To compare two builds, run it once per library and per FDM_GEMM_TILE setting (the library reads that variable once per process)
and diff the outputs:
    FDM_LIB_PATH=<old libfdm_hip.so> python tools/tile_picks.py > old.txt;  python tools/tile_picks.py > new.txt;  diff old.txt new.txt
    FDM_GEMM_TILE=3 ... (the same two runs with the override set)"""
import ctypes as C
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "face-diffusion-model_amd"))
from fdm_amd import _lib  # noqa: E402

MS = (1, 64, 100, 200, 249, 400, 600, 800, 1024, 1200, 1600, 1992, 2400, 3200, 4000, 6400)
NS = (64, 128, 192, 256, 512, 1024, 1536, 2048, 3072, 4096)
KS = (64, 512, 1024, 2048)
BATCHES = (0, 2, 8)
# form name -> fields set on top of the shape (ln_stat_in: any non-null pointer, the query does not read through it)
FORMS = (("plain", {}), ("sched_fuse", {"sched_fuse": 1}), ("sched_fuse+ln", {"sched_fuse": 1, "ln_stat_in": 16}),
         ("ksplit2", {"ksplit": 2}), ("batch2x4", {"batch2": 4, "batch": 16}))


def main():
    l = _lib.lib()
    n = 0
    for (name, dtype), M, N, K, batch, (form, fields) in itertools.product(
            (("f32", _lib.F32), ("bf16", _lib.BF16), ("f16x3", _lib.F16X3), ("f16", _lib.F16)), MS, NS, KS, BATCHES, FORMS):
        a = _lib.GemmArgs()
        a.dtype, a.M, a.N, a.K, a.batch = dtype, M, N, K, batch
        for k, v in fields.items():
            setattr(a, k, v)
        print(f"{name} M={M} N={N} K={K} batch={a.batch} {form}: {l.fdm_gemm_heuristic_tile(C.byref(a))}")
        n += 1
    print(f"# {n} points, FDM_GEMM_TILE={os.environ.get('FDM_GEMM_TILE', '')}")


if __name__ == "__main__":
    main()
