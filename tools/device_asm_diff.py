"""Compare the gfx950 device code of every HIP translation unit between a git revision and the working tree.

    python tools/device_asm_diff.py [REV] [TU ...]      (REV defaults to HEAD, the TUs to every .hip source)

Each .hip source of restartsqp_amd/csrc is compiled with the library's flags plus --offload-device-only -S on both
sides. The assembly is split per function (from `.type <sym>,@function` to `.Lfunc_end`, with the `.amdhsa_kernel`
descriptor block of a kernel appended), comments are dropped and local labels are renumbered per function (removing
one kernel shifts the numbers of the ones after it), and the functions are compared by symbol. Prints, per TU, the
functions only on one side and every function present on both sides whose code or descriptor differs. A symbol removed
from exactly one TU and added to exactly one other has moved: the two texts are compared and it is reported as "moved,
identical" or "moved, CHANGED". The TUs are never merged into one table (qp_small.hip and qp_small_hbm.hip define
equally named, different functions in their anonymous namespaces). Exit status 1 if any function is new, changed or
moved with a change. A refactor that deletes dead kernels shows only removals."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "restartsqp_amd/csrc"
INCLUDE = "include"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-Wno-unused-result", "-x", "hip", "--offload-device-only", "-S"]
_LOCAL = re.compile(r"\.(LBB|Ltmp|Lfunc_end|Lfunc_begin)(\d+)(_\d+)?")


def emit(tree, tu, out):
    subprocess.check_call([HIPCC] + FLAGS + [os.path.join(tree, CSRC, tu), "-o", out], stderr=subprocess.DEVNULL)
    return out


def functions(path):
    """{symbol: normalised text} of one .s file"""
    lines = open(path).read().splitlines()
    funcs, desc = {}, {}
    cur, body = None, []
    kern, kbody = None, []
    for ln in lines:
        m = re.match(r"\s*\.type\s+([^,]+),@function", ln)
        if m:
            cur, body = m.group(1), []
        if cur is not None:
            body.append(ln)
            if re.match(r"\.Lfunc_end\d+:", ln.strip()):
                funcs[cur] = body
                cur = None
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            kern, kbody = m.group(1), []
        if kern is not None:
            kbody.append(ln)
            if ln.strip() == ".end_amdhsa_kernel":
                desc[kern] = kbody
                kern = None
    out = {}
    for sym, body in funcs.items():
        names = {}

        def ren(mm):
            key = mm.group(0)
            if key not in names:
                names[key] = ".%s@%d" % (mm.group(1), len(names))
            return names[key]
        text = [_LOCAL.sub(ren, ln.split(";")[0].rstrip()) for ln in body + desc.get(sym, [])]
        out[sym] = "\n".join(text)
    return out


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    only = set(sys.argv[2:])
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "old")
        os.makedirs(old)
        subprocess.check_call("git -C %s archive %s %s %s | tar -x -C %s" % (ROOT, rev, CSRC, INCLUDE, old), shell=True)
        tus = sorted(set(f for f in os.listdir(os.path.join(old, CSRC)) if f.endswith(".hip")) |
                     set(f for f in os.listdir(os.path.join(ROOT, CSRC)) if f.endswith(".hip")))
        tus = [tu for tu in tus if not only or tu in only]
        jobs = []
        for tu in tus:
            for side, tree in (("old", old), ("new", ROOT)):
                if os.path.exists(os.path.join(tree, CSRC, tu)):
                    jobs.append((tree, tu, os.path.join(tmp, "%s.%s.s" % (tu, side))))
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            list(ex.map(lambda j: emit(*j), jobs))
        old_f, new_f = {}, {}
        for tu in tus:
            po, pn = (os.path.join(tmp, "%s.%s.s" % (tu, s)) for s in ("old", "new"))
            old_f[tu] = functions(po) if os.path.exists(po) else {}
            new_f[tu] = functions(pn) if os.path.exists(pn) else {}
        # a symbol that left exactly one TU and arrived in exactly one other: {symbol: (from, to)}
        left, came = {}, {}
        for tu in tus:
            for sym in set(old_f[tu]) - set(new_f[tu]):
                left.setdefault(sym, []).append(tu)
            for sym in set(new_f[tu]) - set(old_f[tu]):
                came.setdefault(sym, []).append(tu)
        moved = {sym: (left[sym][0], came[sym][0]) for sym in left if len(left[sym]) == 1 and len(came.get(sym, [])) == 1}
        bad = False
        for tu in tus:
            fo, fn = old_f[tu], new_f[tu]
            gone = sorted(sym for sym in set(fo) - set(fn) if sym not in moved)
            added = sorted(sym for sym in set(fn) - set(fo) if sym not in moved)
            changed = sorted(sym for sym in set(fo) & set(fn) if fo[sym] != fn[sym])
            out = sorted(sym for sym in fo if sym in moved and moved[sym][0] == tu)
            into = sorted(sym for sym in fn if sym in moved and moved[sym][1] == tu)
            print("%-16s %4d functions, %d identical, %d removed, %d added, %d changed, %d moved out, %d moved in" %
                  (tu, len(fo), len(set(fo) & set(fn)) - len(changed), len(gone), len(added), len(changed), len(out), len(into)))
            for tag, syms in (("removed", gone), ("added", added), ("CHANGED", changed)):
                for sym in syms:
                    print("    %s %s" % (tag, sym))
            for sym in into:
                same = old_f[moved[sym][0]][sym] == fn[sym]
                print("    moved, %s %s (from %s)" % ("identical" if same else "CHANGED", sym, moved[sym][0]))
                bad |= not same
            bad |= bool(added or changed)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
