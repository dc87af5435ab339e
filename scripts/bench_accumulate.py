#!/usr/bin/env python3
"""What gradient accumulation costs (csrc/accumulate.hip, `hps.optim.accumulate_steps`), at config B (celeba profile: 64x64x3, L 3,
K 32, hidden 512: 44 M parameters), IN ONE PROCESS.

Part 1 -- the combine kernel on the plan's own flat gradient buckets, alternating between
  (a) glowhip_grad_accumulate FIRST / ADD / FINISH through the C ABI (one launch for all buckets)
  (b) torch.add(acc, g, out=acc) over the same buckets (one launch per bucket)
  (c) dst.copy_(src) of the same bytes, a device-to-device copy
HIP events around blocks of calls, warm-up first, min / median / max of the per-round means; GB/s from the bytes the operation must
move (12 per element for ADD, FINISH and (b), 8 for FIRST and (c)), and each mode's rate as a fraction of (c)'s.

Part 2 -- `TrainLoop(graph=True)` and `graph=False` at effective batch 64 run as k = 1, 2, 4, 8 micro-batches, one loop after the
other (so that each has the allocator's peak to itself): ms per optimiser step, images / s, peak `torch.cuda.max_memory_allocated()`
over the timed steps (a replayed graph allocates nothing the allocator sees, so for the captured loops `max_memory_reserved()`,
which holds the graph's private pool, is the figure), host ms per step (a host clock around the calls, no synchronise inside: the
loop's own back-pressure -- it runs at most two steps ahead of the device -- is in it) and the process's CPU ms per step.  On a tree without the
entry point (the parent commit) only k = 1 runs -- the same code, so the two trees can be compared on one box.

Prints ONE JSON line; fails without a GPU.  `--merge parent=FILE ... new=FILE ... --out profiles/accumulate_bench.json` (no GPU)
combines the lines of several runs into the committed record and evaluates the two acceptance conditions: ADD is not slower than (b)
by more than (b)'s own min-max spread over the rounds, and k = 1 on this tree lies within the parent's run-to-run spread."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import _lib, training  # noqa: E402
from pytorch_glow_amd.misc import util  # noqa: E402

DEV = "cuda:0"
HAS_ACC = "glowhip_grad_accumulate" in _lib.SIGNATURES


def make(batch, accumulate=1, seed=0):
    hps = util.load_profile("celeba")
    hps.optim.num_batch_train = batch
    hps.device.graph = [DEV]
    if accumulate > 1:
        hps.optim.accumulate_steps = accumulate
    torch.manual_seed(seed)
    np.random.seed(seed)
    glow = G.Glow(hps)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():      # zero-init tails would make the coupling trivial (as bench.py)
        for name, p in glow.named_parameters():
            if ".f.4." in name or "conv2d_zeros" in name:
                p.copy_(torch.randn(p.shape, generator=g) * 0.002)
    return glow.to(DEV), hps


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def summary(v):
    return {"min_ms": round(min(v), 4), "median_ms": round(statistics.median(v), 4), "max_ms": round(max(v), 4), "rounds": len(v)}


def kernel_workload(args, flats):
    """(a), (b), (c) over one set of flat buffers, alternating."""
    elements = sum(f.numel() for f in flats)
    accs = [torch.randn_like(f) * 0.01 for f in flats]
    spare = [torch.empty_like(f) for f in flats]
    lib = _lib.lib()
    stream = lambda: _lib.stream_ptr(torch.device(DEV))
    variants = {}
    if HAS_ACC:
        table = (_lib.GradSeg * len(flats))(*[_lib.GradSeg(f.data_ptr(), a.data_ptr(), f.numel()) for f, a in zip(flats, accs)])
        call = lambda mode, scale: (lambda i: _lib.check(lib.glowhip_grad_accumulate(table, len(table), mode, scale, stream())))
        variants.update(a_first=call(_lib.ACC_FIRST, 1.0), a_add=call(_lib.ACC_ADD, 1.0), a_finish=call(_lib.ACC_FINISH, 0.5))

    def torch_add(i):
        for f, a in zip(flats, accs):
            torch.add(a, f, out=a)

    def copy(i):
        for f, s in zip(flats, spare):
            s.copy_(f)

    variants.update(b_torch_add=torch_add, c_copy=copy)
    nbytes = {"a_first": 8, "a_add": 12, "a_finish": 12, "b_torch_add": 12, "c_copy": 8}
    with torch.no_grad():
        for fn in variants.values():
            for i in range(args.warmup):
                fn(i)
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                if k == "a_add" or k == "b_torch_add":      # (keep the running sums small: the values never reach inf)
                    for a in accs:
                        a.mul_(0.0)
                ms[k].append(timed(fn, args.kernel_steps))
    med = statistics.median
    gbps = {k: round(nbytes[k] * elements / (med(v) * 1e-3) / 1e9, 1) for k, v in ms.items()}
    out = {"elements": elements, "buckets": len(flats), "calls_per_variant": args.rounds * args.kernel_steps,
           "ms": {k: summary(v) for k, v in ms.items()}, "bytes_per_element": {k: nbytes[k] for k in ms}, "GBps_at_median": gbps,
           "fraction_of_copy_rate": {k: round(gbps[k] / gbps["c_copy"], 3) for k in gbps if k.startswith("a_")},
           "b_torch_add_spread_ms": round(max(ms["b_torch_add"]) - min(ms["b_torch_add"]), 4)}
    if HAS_ACC:
        out["a_add_minus_b_torch_add_ms"] = round(med(ms["a_add"]) - med(ms["b_torch_add"]), 4)
        out["add_not_slower_than_torch_add_beyond_its_spread"] = out["a_add_minus_b_torch_add_ms"] <= out["b_torch_add_spread_ms"]
    return out


def kernel_part(args):
    """Part 1.  The buckets are those of one real training step of the config-B model (batch 4: their sizes do not depend on it).
    `small`: the first 3 M elements of the largest bucket -- the size of a small model's gradient set, cache-resident, a launch
    short enough for its fixed cost to show (recorded, not gated)."""
    glow, _ = make(4)
    glow.train()
    glow.set_actnorm_inited()
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        glow.loss_and_grads(x)
    flats = glow.flow.plan_for(x)._pgrad[0]
    for f in flats:      # (the slot padding is never written by the sweep: give every word a normal value)
        f.copy_(torch.randn(f.shape, device=DEV) * 0.01)
    out = kernel_workload(args, flats)
    out["small"] = kernel_workload(args, [max(flats, key=lambda f: f.numel())[:3_000_000]])
    return out


def train_part(args):
    """Part 2: one loop at a time."""
    x = torch.rand(args.batch, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    out = {}
    for graph in (True, False):
        for k in ([1, 2, 4, 8] if HAS_ACC else [1]):
            loop = training.TrainLoop(*make(args.batch, accumulate=k), graph=graph)
            for _ in range(max(args.warmup, training.TrainLoop.GRAPH_AFTER + 3)):
                loop.step(x)
            torch.cuda.synchronize()
            assert loop.graph_error is None, loop.graph_error
            torch.cuda.reset_peak_memory_stats()
            resident = torch.cuda.memory_allocated()
            ms, host, cpu = [], [], []
            for _ in range(args.rounds):
                t0, c0 = time.perf_counter(), time.process_time()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    loop.step(x)
                e1.record()
                host.append(1e3 * (time.perf_counter() - t0) / args.steps)
                cpu.append(1e3 * (time.process_time() - c0) / args.steps)
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / args.steps)
            peak, reserved = torch.cuda.max_memory_allocated(), torch.cuda.max_memory_reserved()
            loop.flush()
            med = statistics.median(ms)
            out[f"{'graphed' if graph else 'eager'}_k{k}"] = {
                "k": k, "micro_batch": args.batch // k, "graph": graph, "captured": loop._graphed is not None, "step_ms": summary(ms),
                "img_per_s_at_median": round(args.batch / (med * 1e-3), 1), "host_ms_per_step_median": round(statistics.median(host), 3),
                "host_cpu_ms_per_step_median": round(statistics.median(cpu), 3),
                "peak_allocated_bytes": peak, "peak_reserved_bytes": reserved, "resident_before_bytes": resident, "range_fallbacks": loop.range_fallbacks,
                "tape_bytes_micro_batch": int(_lib.lib().glowhip_plan_tape_bytes(loop.glow.flow.plan_for(x)._h, args.batch // k))}
            del loop
            torch.cuda.empty_cache()
    return out


def merge(items, out_path):
    """`items`: "parent=FILE" / "new=FILE" in the order the runs were made; every FILE holds one JSON line of this script."""
    runs, order = {"parent": [], "new": []}, []
    for item in items:
        kind, _, path = item.partition("=")
        if kind not in runs or not path:
            raise SystemExit(f"--merge takes parent=FILE or new=FILE, not {item!r}")
        with open(path) as f:
            runs[kind].append(json.loads(f.read().strip().splitlines()[-1]))
        order.append(kind)
    par, new = runs["parent"], runs["new"]
    if not par or not new:
        raise SystemExit("--merge needs at least one parent= and one new= run")
    med = statistics.median
    comparisons = {
        "part1_a_add_minus_b_torch_add_ms": [r["kernel"]["a_add_minus_b_torch_add_ms"] for r in new],
        "part1_b_torch_add_spread_ms": [r["kernel"]["b_torch_add_spread_ms"] for r in new],
        "part1_add_not_slower_than_torch_add_beyond_its_spread": all(r["kernel"]["add_not_slower_than_torch_add_beyond_its_spread"] for r in new),
    }
    for key in ("graphed_k1", "eager_k1"):
        p = [r["train"][key]["step_ms"]["median_ms"] for r in par if key in r.get("train", {})]
        n = [r["train"][key]["step_ms"]["median_ms"] for r in new if key in r.get("train", {})]
        if not p or not n:
            continue
        # the parent's run-to-run spread: between its runs, and over the rounds inside each of them
        spread = max(max(p) - min(p), max(r["train"][key]["step_ms"]["max_ms"] - r["train"][key]["step_ms"]["min_ms"] for r in par))
        comparisons[key] = {"parent_runs_ms": p, "this_change_runs_ms": n, "parent_run_to_run_spread_ms": round(spread, 4),
                            "this_change_minus_parent_median_ms": round(med(n) - med(p), 4),
                            "within_parent_spread": med(n) - med(p) <= spread}
    first = new[0]
    out = {
        "bench": "accumulate", "script": "scripts/bench_accumulate.py, one process per run, then scripts/bench_accumulate.py --merge",
        "how": "processes on one box in the order " + ", ".join(order) + " (parent = the parent commit's tree with this script); "
               "`comparisons` is computed by --merge from `runs`",
        "device": first["device"], "config": first["config"], "batch": first["batch"],
        "kernel": first["kernel"], "train": first.get("train", {}), "comparisons": comparisons, "runs": runs,
    }
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(comparisons))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs="+", metavar="KIND=FILE", help="combine finished runs (parent=FILE / new=FILE) instead of measuring")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulate_bench.json"), help="where --merge writes")
    ap.add_argument("--batch", type=int, default=64, help="effective (local) batch of every training variant")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=15, help="timed training steps per variant and round")
    ap.add_argument("--kernel-steps", type=int, default=100, help="timed calls per kernel variant and round")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    if not torch.cuda.is_available():
        print("bench_accumulate.py: no GPU visible", file=sys.stderr)
        return 2
    out = {"bench": "accumulate", "device": torch.cuda.get_device_name(0), "config": "B (64x64x3 L3 K32 hidden 512)",
           "has_accumulate_entry_point": HAS_ACC, "batch": args.batch, "lib": os.path.basename(_lib.LIB_PATH)}
    if not args.skip_kernel:
        out["kernel"] = kernel_part(args)
        torch.cuda.empty_cache()
    if not args.skip_train:
        out["train"] = train_part(args)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
