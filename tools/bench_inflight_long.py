"""Long requests in slot mode (fdm_slot_admit_long) measured at the plan level, synthetic weights and audio features, one diffusion
step timed by device events over graph replays (as tools/bench_inflight.py times its steps):

  plain   a slot plan holding plain clips only: without long capacity, and with capacity reserved (the scheduler pass then also
          walks an empty arena).  --parent-tree <a built checkout of the parent commit> adds the parent build's figure for the plan
          without capacity; the three are measured in child processes that alternate, `--rounds` times each.
  group   a 3000-frame request (6 windows of 600, overlap 60) as a group: alone in 6 slots against fdm_sample_windows on the same
          rows, and beside two plain 600-frame clips in 8 slots.
  arrive  one 3000-frame request arriving into a server busy with 500-frame requests (8 slots, DDIM 50), served in flight against
          drain - run alone (fdm_sample_windows) - reopen.  Denoiser + scheduler only: the audio encoder and the VQ stages cost the
          same both ways and are left out.

    python tools/bench_inflight_long.py --out profiles/inflight_long/bench_bf16.json [--parent-tree DIR]

One JSON document."""
import argparse
import json
import os
import subprocess
import sys

# FDM_BENCH_TREE: import the package of another checkout (the parent commit's, for the child that measures its build)
ROOT = os.environ.get("FDM_BENCH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "face-diffusion-model_amd")):
    sys.path.insert(0, p)

DEV = "cuda:0"
PRESET, L, OVERLAP, LONG = "vocaset", 600, 60, 3000


def event_ms(fn, reps):
    """Median over `reps` of the device time of fn() (events on the current stream)."""
    import torch
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def make_plan(dtype):
    from fdm_amd._lib import DTYPE_NAMES
    from fdm_amd.denoiser import DenoiserPlan
    from oracle import weights as W
    return DenoiserPlan(PRESET, W.make_fdm_weights(PRESET), DTYPE_NAMES[dtype], DEV), W


def fill_plain(plan, W, slots, frames, steps, **kw):
    inp = W.synth_inputs(PRESET, len(slots), frames, seed=1)
    plan.open_slots(kw.pop("n_slots"), L, "ddim", steps=steps, **kw)
    for i, s in enumerate(slots):
        plan.admit(s, inp["hub"][i], inp["style"][i], None, inp["x"][i], L=frames)


def child_plain(a):
    """Per-step time of 8 plain 600-frame slots, every slot live.  Under the parent library only the plan without capacity runs."""
    plan, W = make_plan(a.dtype)
    steps, n = 1000, 40                      # chains far longer than the timed window: every slot stays live
    res = {}
    for name, kw in (("no_capacity", {}), ("capacity", dict(long_frames=LONG, long_groups=2))):
        if kw and a.child == "plain_parent":
            continue
        fill_plain(plan, W, list(range(8)), L, steps, n_slots=8, graph_steps=10, **kw)
        plan.run(n)                          # record + instantiate + warm
        res[name + "_ms_per_step"] = event_ms(lambda: plan.run(n), 5) / n
        res[name + "_launches"] = plan.get("launches_per_step")
    print(json.dumps(res))


def long_clip(W):
    inp = W.synth_inputs(PRESET, 1, LONG, seed=2)
    return inp


def group_case(a):
    import torch
    from fdm_amd.denoiser import window_starts
    plan, W = make_plan(a.dtype)
    lc, n, steps = long_clip(W), 40, 1000
    nw = len(window_starts(LONG, L, OVERLAP))
    x = lc["x"].to(DEV)
    plan.prepare_windows(lc["hub"], lc["style"], L_total=LONG, window=L, overlap=OVERLAP)
    plan.sample_windows(x, "ddim", steps=n + 1)
    res = dict(windows=nw, windowed_ms_per_step=event_ms(lambda: plan.sample_windows(x, "ddim", steps=n + 1), 5) / n,
               windowed_launches=plan.get("launches_per_step"), windowed_rows=plan.get("rows"))
    for name, n_slots, plain in (("group_alone", nw, 0), ("group_beside_2_plain", nw + 2, 2)):
        fill_plain(plan, W, list(range(nw, nw + plain)), L, steps, n_slots=n_slots, graph_steps=10, long_frames=LONG, long_groups=1)
        plan.admit_long(list(range(nw)), lc["hub"][0], lc["style"][0], None, lc["x"][0], L_total=LONG, overlap=OVERLAP)
        plan.run(n)
        res[name + "_ms_per_step"] = event_ms(lambda: plan.run(n), 5) / n
        res[name + "_launches"] = plan.get("launches_per_step")
        res[name + "_rows"] = plan.get("rows")
    torch.cuda.synchronize()
    return res


def arrive_case(a):
    """8 slots, DDIM 50 (49 live steps).  Eight 500-frame requests are mid-chain (admitted 6 steps apart) when the long request
    arrives; a new 500-frame request replaces every one that leaves, so the server never idles."""
    import time
    import torch
    from fdm_amd._lib import SLOT_FINISHED
    from fdm_amd.denoiser import window_starts
    plan, W = make_plan(a.dtype)
    lc, steps, short = long_clip(W), 50, 500
    nw = len(window_starts(LONG, L, OVERLAP))
    sh = W.synth_inputs(PRESET, 1, short, seed=3)
    x = lc["x"].to(DEV)

    def admit_short(s):
        plan.admit(s, sh["hub"][0], sh["style"][0], None, sh["x"][0], L=short)

    def serve(in_flight):
        """Returns (seconds until the long request is done, short requests finished by then)."""
        plan.open_slots(8, L, "ddim", steps=steps, long_frames=LONG if in_flight else 0, long_groups=1)
        chain = plan.slot_state(0)[1]
        for s in range(8):                                       # a busy server: slot s is 6 s steps into its chain
            admit_short(s)
            plan.run(6)
        torch.cuda.synchronize()
        t0, done_short, waiting, lead = time.perf_counter(), 0, True, None
        while True:
            for s in range(8):                                   # plain requests that finished leave
                if plan.slot_group(s)[0] < 0 and plan.slot_state(s)[2] == SLOT_FINISHED:
                    plan.read_slot(s, short)
                    done_short += 1
            if not in_flight:                                    # drain, run alone, reopen
                if any(plan.slot_state(s)[2] == 1 for s in range(8)):
                    plan.run(1)
                    continue
                plan.prepare_windows(lc["hub"], lc["style"], L_total=LONG, window=L, overlap=OVERLAP)
                plan.sample_windows(x, "ddim", steps=steps)
                plan.open_slots(8, L, "ddim", steps=steps)
                break
            idle = [s for s in range(8) if plan.slot_state(s)[2] == 0]
            if waiting and len(idle) >= nw:                       # the head of the queue: nothing passes it
                plan.admit_long(idle[:nw], lc["hub"][0], lc["style"][0], None, lc["x"][0], L_total=LONG, overlap=OVERLAP)
                waiting, lead, idle = False, idle[0], idle[nw:]
            if not waiting:
                for s in idle:
                    admit_short(s)
            if lead is not None and plan.slot_state(lead)[2] == SLOT_FINISHED:
                plan.read_long(lead)
                break
            plan.run(1)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, done_short, chain
    res = {}
    for name, mode in (("drain_alone_reopen", False), ("in_flight", True)):
        serve(mode)                                              # record, instantiate, warm
        t, n_short, chain = serve(mode)
        res[name] = dict(seconds_until_long_done=t, short_requests_finished_meanwhile=n_short, chain_steps=chain)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="plain,group,arrive")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child_plain(a)
    doc = dict(preset=PRESET, dtype=a.dtype, slot_frames=L, overlap=OVERLAP, long_frames=LONG)
    cases = a.cases.split(",")
    if "plain" in cases:                                         # alternating fresh child processes, one build each
        runs = []
        for r in range(a.rounds):
            for who in ("this", "parent"):
                if who == "parent" and not a.parent_tree:
                    continue
                env = dict(os.environ)
                if who == "parent":
                    env["FDM_BENCH_TREE"] = os.path.abspath(a.parent_tree)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--dtype", a.dtype, "--child", "plain_" + who], env=env,
                                     capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    raise SystemExit(f"child {who} failed ({out.returncode}): {out.stderr[-2000:]}")
                runs.append(dict(build=who, round=r, **json.loads(out.stdout.strip().splitlines()[-1])))
        doc["plain"] = runs
    if "group" in cases:
        doc["group"] = group_case(a)
    if "arrive" in cases:
        doc["arrive"] = arrive_case(a)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
