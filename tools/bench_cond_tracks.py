"""Condition tracks, measured at the plan level (synthetic weights and audio features), two same-build comparisons:

  admit: the wall time of one admit into an idle slot, fdm_slot_admit_as (one vector per clip: small_linear x 2-3, add_rows, memset)
         against fdm_slot_admit_tracks (one vector per frame: one cond_rows launch), for a 100-frame clip and for a 600-frame clip;
  step:  ms per diffusion step of an 8-slot session whose slots were admitted with tracks against the same session admitted per
         clip -- the same recorded program, so the two should not differ.

The arms alternate inside one process, `--rounds` times, and the medians are reported with the spread of each arm.

    python tools/bench_cond_tracks.py --out profiles/cond_tracks/bench_bf16.json

One JSON document; times are wall clock around stream synchronisation."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "face-diffusion-model_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from fdm_amd._lib import DTYPE_NAMES  # noqa: E402
from fdm_amd.denoiser import DenoiserPlan  # noqa: E402
from oracle import weights as W  # noqa: E402

DEV = "cuda:0"


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=sorted(DTYPE_NAMES))
    ap.add_argument("--preset", default="vocaset")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50, help="live steps of every chain of the step comparison")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    plan = DenoiserPlan(a.preset, W.make_fdm_weights(a.preset), DTYPE_NAMES[a.dtype], DEV)
    p = plan.p
    res = dict(preset=a.preset, dtype=a.dtype, slots=a.slots, rounds=a.rounds, admit_ms={}, step_ms={})

    def clip(L, seed):
        c = W.synth_inputs(a.preset, 1, L, seed=seed)
        c = {k: v.to(DEV) for k, v in c.items()}
        c["st"] = c["style"].expand(L, -1).contiguous()
        c["et"] = c["emo"].expand(L, -1).contiguous() if p.n_emo else None
        return c

    def admit(slot, c, L, with_tracks):
        emo = c["emo"][0] if p.n_emo else None
        if with_tracks:
            plan.admit(slot, c["hub"][0], x_T=c["x"][0], L=L, style_track=c["st"], emotion_track=c["et"])
        else:
            plan.admit(slot, c["hub"][0], c["style"][0], emo, c["x"][0], L=L, sampler=0, cfg_scale=2.5)      # fdm_slot_admit_as

    # admit: one clip into slot 0 of an otherwise idle session, the chain run to its end in between (untimed)
    for L in (100, 600):
        n = plan.open_slots(a.slots, L, kind="ddim", steps=2, cfg=bool(p.n_emo))
        c = clip(L, 3)
        t = {False: [], True: []}
        for r in range(a.rounds + 1):
            for arm in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                admit(0, c, L, arm)
                torch.cuda.synchronize()
                if r:                              # round 0 warms both arms
                    t[arm].append((time.perf_counter() - t0) * 1e3)
                plan.run(n)
                plan.read_slot(0, L)
        res["admit_ms"][f"L{L}"] = dict(per_clip=stats(t[False]), tracks=stats(t[True]))
    # step: every slot live in every timed step
    L = 100
    n = plan.open_slots(a.slots, L, kind="ddim", steps=a.steps + 1, cfg=bool(p.n_emo))
    clips = [clip(L, 10 + s) for s in range(a.slots)]
    t = {False: [], True: []}
    for r in range(a.rounds + 1):
        for arm in (False, True):
            for s in range(a.slots):
                admit(s, clips[s], L, arm)
            plan.run(1)                            # (instantiates the graph on the first round)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plan.run(n - 2)
            torch.cuda.synchronize()
            if r:
                t[arm].append((time.perf_counter() - t0) * 1e3 / (n - 2))
            plan.run(1)
            for s in range(a.slots):
                plan.read_slot(s, L)
    res["step_ms"] = dict(per_clip=stats(t[False]), tracks=stats(t[True]), launches_per_step=plan.get("launches_per_step"), rows=a.slots * L)
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
