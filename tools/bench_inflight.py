"""In-flight batching (slot mode of the denoiser plan) measured at the plan level, synthetic weights and audio features:

  (a) per-step cost of the slot program with every slot live against the plain DDIM program of the same build and shape
      (default cfg2's: 4 x 200 frames, bf16), launch counts, and the cost of one fdm_slot_admit;
  (b) a seeded arrival trace (requests of 100-500 frames arriving every few diffusion steps, DDIM 100) served three ways:
      sequential single-clip sampling, wait-and-batch groups of 8 (padded to the longest clip), and 8 slots.  Denoiser + scheduler
      only: the audio encoder and the VQ stages cost the same in all three and are left out.

    python tools/bench_inflight.py --out profiles/inflight/bench_inflight_bf16.json

One JSON document; times are wall clock around stream synchronisation.  The parent-build comparison of the plain programs is
tools/bench_samplers.py --parent-tree (alternating child processes)."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "face-diffusion-model_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from fdm_amd._lib import DTYPE_NAMES, SLOT_FINISHED  # noqa: E402
from fdm_amd.denoiser import DenoiserPlan  # noqa: E402
from oracle import weights as W  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps=3):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2]


def per_step(plan, preset, B, L, steps):
    inp = W.synth_inputs(preset, B, L, seed=1)
    x = inp["x"].to(DEV)
    plan.prepare(inp["hub"], inp["style"], L=L)
    plan.sample_ddim(x, steps)                                   # record + instantiate
    plain = timed(lambda: plan.sample_ddim(x, steps))
    n_live = steps - 1
    res = dict(plain_ms_per_step=1e3 * plain / n_live, plain_launches=plan.get("launches_per_step"))

    def session():
        plan.open_slots(B, L, "ddim", steps=steps)
        for b in range(B):
            plan.admit(b, inp["hub"][b], inp["style"][b], None, inp["x"][b], L=L)
    session()
    plan.run(n_live)                                             # record + instantiate
    ts = []
    for _ in range(3):
        session()
        ts.append(timed(lambda: plan.run(n_live), reps=1))
    res.update(slot_ms_per_step=1e3 * sorted(ts)[1] / n_live, slot_launches=plan.get("launches_per_step"))
    res["slot_minus_plain_us_per_step"] = 1e3 * (res["slot_ms_per_step"] - res["plain_ms_per_step"])
    # one admit into an idle slot while the others hold clips (stream-ordered GEMMs + copies; the slot is reopened every time)
    ad = []
    for _ in range(5):
        plan.open_slots(B, L, "ddim", steps=steps)
        ad.append(timed(lambda: plan.admit(0, inp["hub"][0], inp["style"][0], None, inp["x"][0], L=L), reps=1))
    res["admit_ms"] = 1e3 * sorted(ad)[2]
    return res


def trace(plan, preset, n_req, steps, gap, seed, slots=8):
    rng = random.Random(seed)
    reqs = [dict(L=rng.randint(100, 500), arrive=i * gap + rng.randint(0, gap)) for i in range(n_req)]
    for r in reqs:
        r.update(W.synth_inputs(preset, 1, r["L"], seed=1000 + r["L"]))
    n_live = steps - 1
    frames = sum(r["L"] for r in reqs)
    # the clock of the trace is the diffusion step of a server that never idles: a request "arrives" at wall time arrive * (time of
    # one 8-slot step), measured first; every strategy starts at the first arrival and may not start a request before it arrives
    Lmax = max(r["L"] for r in reqs)
    plan.open_slots(slots, Lmax, "ddim", steps=steps)
    for s in range(slots):
        r = reqs[s % n_req]
        plan.admit(s, r["hub"][0], r["style"][0], None, r["x"][0], L=r["L"])
    plan.run(n_live)
    plan.open_slots(slots, Lmax, "ddim", steps=steps)
    tick = timed(lambda: plan.run(10), reps=3) / 10
    out = dict(requests=n_req, frames=frames, ddim_steps=steps, tick_ms=1e3 * tick)

    def report(name, t_done, t_total):
        lat = [t_done[i] - reqs[i]["arrive"] * tick for i in range(n_req)]
        out[name] = dict(makespan_s=t_total, frames_per_s=frames / t_total, mean_completion_s=sum(lat) / n_req, worst_completion_s=max(lat))

    def wait_until(t0, t):
        while time.perf_counter() - t0 < t:
            pass

    # (i) sequential single-clip sampling
    t0, done = time.perf_counter(), {}
    for i, r in enumerate(reqs):
        wait_until(t0, r["arrive"] * tick)
        plan.prepare(r["hub"], r["style"], L=r["L"])
        plan.sample_ddim(r["x"].to(DEV), steps)
        torch.cuda.synchronize()
        done[i] = time.perf_counter() - t0
    report("sequential", done, max(done.values()))
    # (ii) wait-and-batch: groups of `slots` in arrival order, each started when its last member has arrived, padded to its longest
    t0, done = time.perf_counter(), {}
    for g0 in range(0, n_req, slots):
        grp = list(range(g0, min(g0 + slots, n_req)))
        wait_until(t0, max(reqs[i]["arrive"] for i in grp) * tick)
        Lg = max(reqs[i]["L"] for i in grp)
        N = Lg * plan.p.pair
        hub = torch.zeros(len(grp), N, reqs[0]["hub"].shape[2])
        x = torch.zeros(len(grp), Lg * plan.p.G, plan.p.c)
        for j, i in enumerate(grp):
            hub[j, :reqs[i]["hub"].shape[1]] = reqs[i]["hub"][0]
            x[j, :reqs[i]["x"].shape[1]] = reqs[i]["x"][0]
        plan.prepare(hub, torch.cat([reqs[i]["style"] for i in grp]), L=Lg)
        plan.sample_ddim(x.to(DEV), steps)
        torch.cuda.synchronize()
        for i in grp:
            done[i] = time.perf_counter() - t0
    report("wait_and_batch", done, max(done.values()))
    # (iii) slots: admit on arrival (at the next boundary of a 5-step run), read when finished
    plan.open_slots(slots, Lmax, "ddim", steps=steps)
    t0, done, queue, where, nxt = time.perf_counter(), {}, [], {}, 0
    while len(done) < n_req:
        now = time.perf_counter() - t0
        while nxt < n_req and reqs[nxt]["arrive"] * tick <= now:
            queue.append(nxt)
            nxt += 1
        for s in range(slots):
            if s not in where and queue:
                i = queue.pop(0)
                r = reqs[i]
                plan.admit(s, r["hub"][0], r["style"][0], None, r["x"][0], L=r["L"])
                where[s] = i
        if not where:
            continue
        plan.run(5)
        fin = [s for s in where if plan.slot_state(s)[2] == SLOT_FINISHED]
        if fin:
            for s in fin:
                plan.read_slot(s, reqs[where[s]]["L"])
            torch.cuda.synchronize()
            for s in fin:
                done[where.pop(s)] = time.perf_counter() - t0
    report("slots", done, max(done.values()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=sorted(DTYPE_NAMES))
    ap.add_argument("--preset", default="vocaset")
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--gap", type=int, default=20, help="mean diffusion steps between arrivals")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    plan = DenoiserPlan(a.preset, W.make_fdm_weights(a.preset), DTYPE_NAMES[a.dtype], DEV)
    res = dict(dtype=a.dtype, preset=a.preset, shape=[a.B, a.L], per_step=per_step(plan, a.preset, a.B, a.L, a.steps))
    if not a.skip_trace:
        res["trace"] = trace(plan, a.preset, a.requests, a.steps, a.gap, a.seed)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
