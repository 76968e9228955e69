"""Samplers per request in slot mode, measured at the plan level (synthetic weights and audio features): ms per diffusion step of an
8-slot session whose slots run THREE samplers at once (DDIM, DPM-Solver++ 2M, DDPM; every chain `--steps` long, so every slot is live
in every timed step) on the bank program, against the same rows on the single-sampler slot program (no bank capacity: the program a
plan records without this feature, all slots on DDIM).  The two arms alternate inside one process, `--rounds` times; the spread of
each arm over the rounds is the run-to-run noise the difference has to be read against.

    python tools/bench_inflight_mixed.py --out profiles/inflight_samplers/bench_mixed_bf16.json

One JSON document; times are wall clock around stream synchronisation."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "face-diffusion-model_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from fdm_amd import schedule  # noqa: E402
from fdm_amd._lib import DTYPE_NAMES  # noqa: E402
from fdm_amd.denoiser import DenoiserPlan  # noqa: E402
from oracle import weights as W  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=sorted(DTYPE_NAMES))
    ap.add_argument("--preset", default="vocaset")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--steps", type=int, default=50, help="live steps of every chain")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    plan = DenoiserPlan(a.preset, W.make_fdm_weights(a.preset), DTYPE_NAMES[a.dtype], DEV)
    inp = W.synth_inputs(a.preset, a.slots, a.L, seed=1)
    K = a.steps
    ddim = dict(kind="ddim", steps=K + 1)                                   # K live pairs
    t2m, tab2m = schedule.sampler_tables("dpmpp2m", K)
    two_m = dict(kind="tables", t_list=t2m, tables=tab2m)
    ddpm = dict(kind="ddpm", t_list=[int(round(999 - i * 998 / (K - 1))) for i in range(K)] if K > 1 else [999])

    def admit_all(ids):
        for b in range(a.slots):
            plan.admit(b, inp["hub"][b], inp["style"][b], None, inp["x"][b], L=a.L, seed=b, clip_id=b, sampler=ids[b % len(ids)])

    def single():
        assert plan.open_slots(a.slots, a.L, **ddim) == K
        admit_all([0])

    def mixed():
        assert plan.open_slots(a.slots, a.L, samplers=2, sampler_steps=2 * K, **ddim) == K
        admit_all([0, plan.add_sampler(**two_m), plan.add_sampler(**ddpm)])

    def timed(session):
        session()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan.run(K)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / K
    launches = {}
    for name, session in (("single", single), ("mixed", mixed)):          # record + instantiate both programs
        timed(session)
        launches[name] = plan.get("launches_per_step")
    ms = {"single": [], "mixed": []}
    for _ in range(a.rounds):
        for name, session in (("single", single), ("mixed", mixed)):
            ms[name].append(timed(session))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    res = dict(dtype=a.dtype, preset=a.preset, slots=a.slots, L=a.L, rows=a.slots * a.L, steps=K, rounds=a.rounds, launches_per_step=launches,
               ms_per_step_median=med, ms_per_step_min={k: min(v) for k, v in ms.items()}, ms_per_step_max={k: max(v) for k, v in ms.items()},
               mixed_minus_single_us=1e3 * (med["mixed"] - med["single"]), ms_per_step_all=ms)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
