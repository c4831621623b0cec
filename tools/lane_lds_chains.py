"""Static view of the lane-per-problem kernel's LDS traffic (qp_lane.hip), per instantiation and per segment between two phase
fences (`sched_barrier(0)`, the product build's LSTAMP): how many LDS reads and writes it holds, how many `s_waitcnt lgkmcnt`,
and how many reads were in flight at each wait. A wait with ONE read issued since the wait before it is a round trip that
nothing overlaps: a lone wave on a SIMD pays its whole latency. `trips` is the longest run of such waits in a row in the
segment's text, `in bb` the longest inside one basic block (the text of a segment holds every path side by side: the blocks of a
conditional path, and blocks of another phase that the compiler laid out here, stand between the ones a wave executes).

Host only: compiles to assembly with build.py's flags, needs no GPU.
    python tools/lane_lds_chains.py [--source FILE | --asm FILE] [extra compiler flags]
(--source: another version of qp_lane.hip, e.g. `git show HEAD~1:restartsqp_amd/csrc/qp_lane.hip` saved beside the headers it
includes; --asm: a file compiled before)"""
import os, re, subprocess, sys, tempfile
from collections import Counter
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from restartsqp_amd import build

FENCE = "sched_barrier mask(0x00000000)"
KERNEL = re.compile(r"^(_ZN\S*lane_qp_(?:shape_)?kernelILi(\d+)ELb([01])ELb([01])ELi(\d+)E(?:Li(\d+)ELi(\d+)E)?\S*):")
USAGE = re.compile(r"remark: +(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)")


def compile_asm(extra, source=None):
    out = os.path.join(tempfile.mkdtemp(prefix="lane_chains_"), "qp_lane.s")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS + extra + \
          ["-x", "hip", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I" + build.CSRC, source or os.path.join(build.CSRC, "qp_lane.hip"), "-o", out]
    err = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, text=True).stderr
    usage, name = {}, None
    for key, val in USAGE.findall(err):
        if key == "Function Name":
            name = val
            usage[name] = []
        elif name is not None:
            usage[name].append("%s %s" % (key.split(" [")[0], val))
    return out, usage


def segments(lines):
    """[(first line, last line, reads, writes, waits, Counter(reads in flight at a wait), longest run of one-read waits, the same
    inside one basic block)]"""
    out, start = [], 0
    reads = writes = waits = since = run = longest = run_bb = longest_bb = 0
    hist = Counter()
    for n, raw in enumerate(lines + ["; " + FENCE]):
        s = raw.strip()
        if FENCE in s:
            out.append((start, n, reads, writes, waits, hist, longest, longest_bb))
            start, reads, writes, waits, since, run, longest, run_bb, longest_bb, hist = n + 1, 0, 0, 0, 0, 0, 0, 0, 0, Counter()
            continue
        if s.startswith(".LBB"):
            run_bb = 0
        op = s.split(None, 1)[0] if s else ""
        if op.startswith("ds_read"):
            reads += 1; since += 1
        elif op.startswith("ds_write"):
            writes += 1
        elif op == "s_waitcnt" and "lgkmcnt" in s:
            waits += 1
            hist[since] += 1
            if since == 1:
                run += 1; longest = max(longest, run)
                run_bb += 1; longest_bb = max(longest_bb, run_bb)
            elif since > 1:
                run = run_bb = 0                                 # (a wait with no read since the last one -- for a store, a scalar load -- leaves a run as it is)
            since = 0
    return out


def main(argv):
    extra, asm, source = [], None, None
    it = iter(argv)
    for a in it:
        if a == "--asm":
            asm = next(it)
        elif a == "--source":
            source = next(it)
        else:
            extra.append(a)
    usage = {}
    if asm is None:
        asm, usage = compile_asm(extra, source)
    lines = open(asm).read().split("\n")
    k = 0
    while k < len(lines):
        m = KERNEL.match(lines[k])
        if not m:
            k += 1
            continue
        end = next(j for j in range(k, len(lines)) if lines[j].startswith(".Lfunc_end"))
        print("lane_qp_%skernel<%s, %s, %s, %s%s>" % ("shape_" if m.group(6) else "", m.group(2), ("false", "true")[int(m.group(3))], ("false", "true")[int(m.group(4))],
                                             m.group(5), ", %s, %s" % (m.group(6), m.group(7)) if m.group(6) else ""))
        if m.group(1) in usage:
            print("    " + "; ".join(usage[m.group(1)]))
        print("    %-4s %-13s %6s %6s %6s %6s %6s   %s" % ("seg", "lines", "reads", "writes", "waits", "trips", "in bb", "reads in flight at a wait: count"))
        tot = [0, 0, 0]
        for s, (a, b, r, w, wt, hist, longest, longest_bb) in enumerate(segments(lines[k:end])):
            tot = [tot[0] + r, tot[1] + w, tot[2] + wt]
            if r + w + wt:
                print("    %-4d %-13s %6d %6d %6d %6d %6d   %s" % (s, "%d-%d" % (a, b), r, w, wt, longest, longest_bb,
                                                                  " ".join("%d:%d" % kv for kv in sorted(hist.items()))))
        print("    all  %-13s %6d %6d %6d" % ("", tot[0], tot[1], tot[2]))
        k = end + 1


if __name__ == "__main__":
    main(sys.argv[1:])
