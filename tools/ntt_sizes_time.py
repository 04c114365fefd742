"""Device-resident timing of the general-N NTT (ntt_sizes.hip) next to its two yardsticks, in one process:
a device copy of the same bytes (tools/copy_bw.py's method) and the N = 1024 kernels on 4096 polynomials.

    python tools/ntt_sizes_time.py [--out-dir profiles] [--reps 9] [--inner 20]

Per N in {512, 2048, 4096, 16384, 65536} and arithmetic width (the largest primes = 1 mod 2N below 2^30 and
2^60), a batch of 32 MiB of polynomials (BASELINE config 2's footprint) is transformed in place.  One
repetition is `inner` back-to-back launches between two device events; after a warm-up, `reps` repetitions
give the median and the spread (min .. max) per launch.  Bytes/s are algorithmic traffic over the median:
16 B per coefficient for a one-pass transform (8 read + 8 written), 32 B for a two-pass one.  The two
largest one-pass sizes (the cut and half of it) are measured both ways, in one pass and, with the plan's
cut moved below them (fhe_hip_ntt_plan_set_onepass_max), in two, alternating repetition by repetition.  Writes ntt_sizes_time.txt and ntt_sizes_time.json."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fhe_amd import FheHipError, NttPlan  # noqa: E402
from fhe_amd.ntt import onepass_max  # noqa: E402

BYTES = 32 << 20


def largest_prime(N, bits):
    """the largest prime = 1 mod 2N below 2^bits: the first candidate the library accepts for a plan"""
    q = ((1 << bits) - 2) // (2 * N) * (2 * N) + 1
    while True:
        try:
            NttPlan(q, N=N).close()
            return q
        except FheHipError as e:
            if e.code != -2:
                raise
            q -= 2 * N


def time_reps(fns, reps, inner):
    """per-launch microseconds of each fn, `reps` repetitions of `inner` launches, the fns alternating"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) / inner * 1e3)
    return us


def summary(us, nbytes):
    med = statistics.median(us)
    return dict(median_us=round(med, 2), min_us=round(min(us), 2), max_us=round(max(us), 2),
                gbytes_per_s=round(nbytes / med / 1e3, 1), bytes=nbytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    assert args.reps >= 7
    # one stream of our own for the launches, the copies and the events (the default stream's handle is
    # NULL, which the C-ABI reads as "the plan's stream")
    ts = torch.cuda.Stream()
    torch.cuda.set_stream(ts)
    stream = ts.cuda_stream
    assert stream
    buf = torch.zeros(BYTES // 8, dtype=torch.int64, device="cuda")
    dst = torch.empty_like(buf)
    rows = []

    def fill(Q):
        g = torch.Generator(device="cuda").manual_seed(1)
        buf.copy_(torch.randint(0, Q, (BYTES // 8,), dtype=torch.int64, device="cuda", generator=g))

    def ntt_case(label, N, Q, cuts):
        """one plan per cut (None: the default), forward and inverse, the cuts alternating"""
        count = BYTES // (8 * N)
        plans = []
        for cut in cuts:
            p = NttPlan(Q, N=N)
            if cut is not None:
                p.set_onepass_max(cut)
            plans.append(p)
        fill(Q)
        for inv in (False, True):
            fns = [lambda p=p: p.run_device(buf.data_ptr(), buf.data_ptr(), count, inv, stream) for p in plans]
            for p, cut, us in zip(plans, cuts, time_reps(fns, args.reps, args.inner)):
                passes = p.dispatch()[0]
                r = dict(case=label, N=N, Q=Q, width=64 if Q >= 1 << 30 else 32, count=count,
                         direction="inverse" if inv else "forward", passes=passes,
                         onepass_max="default" if cut is None else cut, bytes_per_coeff=16 * passes,
                         **summary(us, 16 * passes * count * N))
                rows.append(r)
                print(r, flush=True)

    copy_us = time_reps([lambda: dst.copy_(buf)], args.reps, args.inner)[0]
    rows.append(dict(case="copy", **summary(copy_us, 2 * BYTES)))
    print(rows[-1], flush=True)
    for bits in (30, 60):
        ntt_case("n1024", 1024, largest_prime(1024, bits), [None])
    for N in (512, 2048, 4096, 16384, 65536):
        for bits in (30, 60):
            ntt_case("sizes", N, largest_prime(N, bits), [None])
    # the cut: the two largest one-pass sizes, each run in one pass (the default) and in two
    for bits in (30, 60):
        cut = onepass_max(bits > 30)
        for N in (cut // 2, cut):
            ntt_case("cut", N, largest_prime(N, bits), [None, N // 2])
    copy_us = time_reps([lambda: dst.copy_(buf)], args.reps, args.inner)[0]
    rows.append(dict(case="copy (end of run)", **summary(copy_us, 2 * BYTES)))

    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "ntt_sizes_time.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=args.reps, inner=args.inner, rows=rows), f, indent=1)
    with open(os.path.join(args.out_dir, "ntt_sizes_time.txt"), "w") as f:
        f.write(f"# {torch.cuda.get_device_name(0)}; per launch, median (min .. max) of {args.reps} repetitions of "
                f"{args.inner} launches; 32 MiB batches in place;\n# GB/s = algorithmic bytes (16 B per coefficient "
                f"and pass; copy: 8 read + 8 written) over the median\n")
        f.write(f"{'case':18} {'N':>6} {'width':>5} {'dir':>8} {'passes':>6} {'cut':>8} {'median us':>10} "
                f"{'min':>8} {'max':>8} {'GB/s':>8}\n")
        for r in rows:
            f.write(f"{r['case']:18} {r.get('N', ''):>6} {r.get('width', ''):>5} {r.get('direction', ''):>8} "
                    f"{r.get('passes', ''):>6} {str(r.get('onepass_max', '')):>8} {r['median_us']:>10.2f} "
                    f"{r['min_us']:>8.2f} {r['max_us']:>8.2f} {r['gbytes_per_s']:>8.1f}\n")


if __name__ == "__main__":
    main()
