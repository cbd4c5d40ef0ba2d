#!/usr/bin/env python3
"""Cost of the filters of the final interval (-M, --max-n, --max-ee) on the bench configuration: device-generated
config-3 pairs (TAKARAV3, 150 nt), pipelined cs_trim_device calls as bench.py issues them; the plan without a filter,
with each filter alone and with all three, alternating.  Prints one JSON line per leg and a summary line: M pairs/s,
scan and resolve kernel ms per call, reads flagged per call and mate.

  python tools/filters_ab.py [--pairs 20000000] [--steps 20] [--warmup 5] [--rounds 3] [--max-length 100] [--max-ee 1]

--ends: the read-end modifiers instead (-q FRONT,BACK and --trim-n): the plan without them, with -q FRONT,20, with
--trim-n and with both, and -- from a sample of the same reads -- the share of reads whose 5' walk leaves the first
quality dword of the interval the trimmer sees (the walk is one lane per read: tools/README.md).

  python tools/filters_ab.py --ends [--front 20] [--sample 1000000]

--nextseq: the cost of --nextseq-trim CUTOFF: the plan without it against the plan with a NextSeqTrimOp in front of the
quality trimmer of both mates.  --only LEG[,LEG]: these legs alone (an A/B of two libraries runs one leg under each,
CUTSEQ_HIP_LIB choosing the library).

  python tools/filters_ab.py --nextseq [--cutoff 20]

--shorten: the cost of -l LENGTH: the plan without it against the plan with a ShortenOp behind the quality trimmer of
both mates.  Without --length the median final length of a sample of the same reads (both mates, the plan without the
op) is taken and printed.

  python tools/filters_ab.py --shorten [--length N] [--sample 1000000]

--poly-a: the headline configuration in three variants -- "trim_polya" (--trim-polyA: the reference's poly-A adapters,
what bench.py times), "poly_a" (--poly-a in their place: cutadapt's PolyATrimmer, CS_OP_POLYA) and "neither" -- with the
bases each poly step removed per call where the engine counts them.

  python tools/filters_ab.py --poly-a
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from cutseq_amd import abi, synth, workloads  # noqa: E402
from cutseq_amd.engine import TrimEngine  # noqa: E402


def plan_for(filters):
    from cutseq_amd import plan as planmod
    tp = workloads.make_plan("config3")
    tp.max_length, tp.max_n, tp.max_ee = filters.get("max_length"), filters.get("max_n"), filters.get("max_ee")
    if filters.get("poly") is not None:  # "trim_polya": the plan as it is; "poly_a": a PolyATrimOp in the adapters' place
        for chain in (tp.r1, tp.r2):
            at = [i for i, o in enumerate(chain.ops) if isinstance(o, planmod.AdapterOp) and o.match_flag == abi.CS_F_POLY]
            assert len(at) == 1
            if filters["poly"] == "poly_a":  # NonInternalFrontAdapter (poly-T head) -> revcomp, as plan.py's strand rule
                chain.ops[at[0]] = planmod.PolyATrimOp(chain.ops[at[0]].kind_name == "NonInternalFrontAdapter")
            elif filters["poly"] == "neither":
                del chain.ops[at[0]]
    for chain in (tp.r1, tp.r2):
        if filters.get("drop_qtrim"):
            chain.ops = [o for o in chain.ops if not isinstance(o, planmod.QTrimOp)]
        for o in chain.ops:
            if isinstance(o, planmod.QTrimOp):
                o.cutoff_front = filters.get("front", 0)
        if filters.get("trim_n"):
            chain.ops = chain.ops + [planmod.NTrimOp()]
        if filters.get("nextseq") is not None:  # immediately in front of the chain's quality trimmer
            at = next(i for i, o in enumerate(chain.ops) if isinstance(o, planmod.QTrimOp))
            chain.ops = chain.ops[:at] + [planmod.NextSeqTrimOp(filters["nextseq"])] + chain.ops[at:]
        if filters.get("shorten") is not None:  # directly behind the chain's quality trimmer, in front of an N trimmer
            at = next(i for i, o in enumerate(chain.ops) if isinstance(o, planmod.QTrimOp))
            chain.ops = chain.ops[:at + 1] + [planmod.ShortenOp(filters["shorten"])] + chain.ops[at + 1:]
    return tp


def median_final_length(d, n, stride):
    """Of the first n pairs: the median length of what the plan without the op leaves (both mates together)."""
    import numpy as np
    dev = torch.device("cuda:0")
    outs = [torch.empty((n, 8), dtype=torch.uint8, device=dev) for _ in range(2)]
    rr = [abi.cs_reads(d[f"seq{m}"].data_ptr(), d[f"qual{m}"].data_ptr(), d[f"len{m}"].data_ptr(), outs[m - 1].data_ptr(),
                       None, None, None) for m in (1, 2)]
    with TrimEngine(plan_for({}), device=0, slots=0) as eng:
        eng.trim_device(rr[0], rr[1], n, stride)
        torch.cuda.synchronize(dev)
    res = [o.cpu().numpy().view(abi.RESULT_DTYPE).reshape(-1) for o in outs]
    return int(np.median(np.concatenate([r["stop"].astype(np.int64) - r["start"].astype(np.int64) for r in res])))


def front_walk_share(d, n, stride, front, base=33):
    """Of the first n pairs: the share of reads (both mates) whose front walk under ``front`` reads more than the first
    quality dword of the interval the trimmer sees -- its sum is not negative anywhere in that dword and the interval
    goes on behind it.  The intervals come from the plan without its quality trimmer."""
    import numpy as np
    dev = torch.device("cuda:0")
    outs = [torch.empty((n, 8), dtype=torch.uint8, device=dev) for _ in range(2)]
    rr = [abi.cs_reads(d[f"seq{m}"].data_ptr(), d[f"qual{m}"].data_ptr(), d[f"len{m}"].data_ptr(), outs[m - 1].data_ptr(),
                       None, None, None) for m in (1, 2)]
    with TrimEngine(plan_for({"drop_qtrim": True}), device=0, slots=0) as eng:
        eng.trim_device(rr[0], rr[1], n, stride)
        torch.cuda.synchronize(dev)
    beyond = total = 0
    for m in (1, 2):
        res = outs[m - 1].cpu().numpy().view(abi.RESULT_DTYPE).reshape(-1)
        q = d[f"qual{m}"][:n].cpu().numpy().astype(np.int64)
        s, e = res["start"].astype(np.int64), res["stop"].astype(np.int64)
        first_end = np.minimum(e, (s | 3) + 1)  # end of the interval's part inside its first dword
        alive = e > s
        run = np.zeros(n, dtype=np.int64)
        for b in range(4):
            p = s + b
            inside = alive & (p < first_end)
            run = np.where(inside, run + front + base - q[np.arange(n), np.minimum(p, stride - 1)], run)
            alive = alive & ~(inside & (run < 0))
        beyond += int((alive & (e > first_end)).sum())
        total += int((e > s).sum())
    return beyond / max(total, 1)


def leg(d, n, stride, filters, steps, warmup, with_xflags):
    tp = plan_for(filters)
    dev = torch.device("cuda:0")
    sets = []
    for _ in range(3):
        o1 = torch.empty((n, 8), dtype=torch.uint8, device=dev)
        o2 = torch.empty((n, 8), dtype=torch.uint8, device=dev)
        x1 = torch.empty(n, dtype=torch.uint8, device=dev) if with_xflags else None
        x2 = torch.empty(n, dtype=torch.uint8, device=dev) if with_xflags else None
        r1 = abi.cs_reads(d["seq1"].data_ptr(), d["qual1"].data_ptr(), d["len1"].data_ptr(), o1.data_ptr(), None, None,
                          x1.data_ptr() if x1 is not None else None)
        r2 = abi.cs_reads(d["seq2"].data_ptr(), d["qual2"].data_ptr(), d["len2"].data_ptr(), o2.data_ptr(), None, None,
                          x2.data_ptr() if x2 is not None else None)
        sets.append((r1, r2, o1, o2, x1, x2))
    with TrimEngine(tp, device=0, slots=0) as eng:
        stream = torch.cuda.Stream(device=dev)
        sh = C.c_void_p(stream.cuda_stream)
        for i in range(warmup):
            eng.trim_device(sets[i % 3][0], sets[i % 3][1], n, stride, stream=sh, pipelined=True)
        eng.join(sh)
        torch.cuda.synchronize(dev)
        eng.stats(reset=True)
        eng.xflag_counts(reset=True)
        eng.kernel_time_totals(reset=True)
        t0 = time.perf_counter()
        for i in range(steps):
            eng.trim_device(sets[i % 3][0], sets[i % 3][1], n, stride, stream=sh, pipelined=True)
        eng.join(sh)
        torch.cuda.synchronize(dev)
        elapsed = time.perf_counter() - t0
        calls, scan_ms, resolve_ms = eng.kernel_time_totals()
        c1, c2 = eng.xflag_counts()
        poly_a_bp = [b // steps for b in eng.polya_bp()] if tp.has_poly_a else None
    return {"filters": filters, **({"poly_a_bp": poly_a_bp} if poly_a_bp is not None else {}), "mpairs_s": n * steps / elapsed / 1e6, "scan_ms": scan_ms / calls,
            "resolve_ms": resolve_ms / calls, "flagged": {k: [c1[k] // steps, c2[k] // steps] for k in c1}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-n", type=float, default=0.0)
    ap.add_argument("--max-length", type=int, default=100)
    ap.add_argument("--max-ee", type=float, default=1.0)
    ap.add_argument("--xflags", action="store_true", help="also write cs_reads.xflags (the text path does)")
    ap.add_argument("--ends", action="store_true", help="the legs of -q FRONT,20 and --trim-n instead of the filters'")
    ap.add_argument("--front", type=int, default=20, help="--ends: the 5' cutoff")
    ap.add_argument("--sample", type=int, default=1_000_000, help="--ends / --shorten: pairs the front-walk share / the median length is counted on")
    ap.add_argument("--nextseq", action="store_true", help="the legs of --nextseq-trim instead of the filters'")
    ap.add_argument("--cutoff", type=int, default=20, help="--nextseq: the cutoff")
    ap.add_argument("--shorten", action="store_true", help="the legs of -l LENGTH instead of the filters'")
    ap.add_argument("--length", type=int, default=None, help="--shorten: the length (default: the median final length)")
    ap.add_argument("--poly-a", dest="poly_a", action="store_true",
                    help="the headline with --trim-polyA, with --poly-a in its place and with neither, instead of the filters' legs")
    ap.add_argument("--only", type=str, default=None, help="run these legs alone (comma-separated)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.pairs
    stride = synth._stride_for(150)
    names = ("seq1", "qual1", "len1", "seq2", "qual2", "len2")
    d = {k: torch.empty((n,) if k.startswith("len") else (n, stride),
                        dtype=torch.int16 if k.startswith("len") else torch.uint8, device=dev) for k in names}
    assert workloads.fill_device("config3", n, [d[k].data_ptr() for k in names]) == stride
    torch.cuda.synchronize(dev)
    legs = (("off", {}), ("max_n", {"max_n": args.max_n}), ("max_length", {"max_length": args.max_length}),
            ("max_ee", {"max_ee": args.max_ee}),
            ("all", {"max_length": args.max_length, "max_n": args.max_n, "max_ee": args.max_ee}))
    if args.ends:
        legs = (("off", {}), ("q_front", {"front": args.front}), ("trim_n", {"trim_n": True}),
                ("both", {"front": args.front, "trim_n": True}))
        share = front_walk_share(d, min(n, args.sample), stride, args.front)
        print(json.dumps({"front_walk_beyond_first_dword": round(share, 5), "front": args.front,
                          "sample_pairs": min(n, args.sample)}), flush=True)
    if args.nextseq:
        legs = (("off", {}), ("nextseq", {"nextseq": args.cutoff}))
    if args.shorten:
        length = args.length
        if length is None:
            length = median_final_length(d, min(n, args.sample), stride)
            print(json.dumps({"median_final_length": length, "sample_pairs": min(n, args.sample)}), flush=True)
        legs = (("off", {}), ("shorten", {"shorten": length}))
    if args.poly_a:  # ("off" is what the summary compares with: the headline as bench.py runs it)
        legs = (("off", {"poly": "trim_polya"}), ("poly_a", {"poly": "poly_a"}), ("neither", {"poly": "neither"}))
    if args.only:
        legs = tuple(leg_ for leg_ in legs if leg_[0] in args.only.split(","))
    res = {key: [] for key, _ in legs}
    for _ in range(args.rounds):
        for key, filters in legs:
            r = leg(d, n, stride, filters, args.steps, args.warmup, args.xflags)
            res[key].append(r)
            print(json.dumps({"leg": key, **r}), flush=True)
    med = {k: {f: statistics.median(x[f] for x in v) for f in ("mpairs_s", "scan_ms", "resolve_ms")} for k, v in res.items()}
    slow = {k: round(100.0 * (1.0 - med[k]["mpairs_s"] / med["off"]["mpairs_s"]), 2) for k in med if k != "off" and "off" in med}
    print(json.dumps({"summary": med, "slowdown_pct": slow, "pairs": n, "steps": args.steps, "rounds": args.rounds}),
          flush=True)


if __name__ == "__main__":
    main()
