"""Is the device code of the HIP sources (default: the fused stack kernels) the same as at another commit?

    python tools/device_asm_diff.py [--base REV] [--rename REGEX=REPL ...] [FILE.hip ...]

Compiles device-only gfx950 assembly (build.FLAGS + ``--cuda-device-only -S``) of csrc/fused_layers.hip,
fused_hoisted.hip and fused_sa.hip (or the named sources) twice: from the working tree, and from ``git archive REV``
(default HEAD~1) unpacked into a temporary directory.  Per ``.amdhsa_kernel`` symbol it compares the instruction text
of the function body and the ``.amdhsa_*`` descriptor block (VGPRs, SGPRs, LDS, scratch); kernels are matched by name
because the order in which templates are emitted depends on the host code that instantiates them.  Basic-block labels
carry the function's position in the file (``.LBB<fn>_<n>``); the position is dropped before comparing.  Comments are
dropped as well.  Exit status 0 and one ``identical`` line per source when nothing differs, 1 otherwise.

``--rename REGEX=REPL`` (repeatable) pairs kernels whose signature changed: symbols are demangled (llvm-cxxfilt or c++filt) and the
substitution is applied to the BASE tree's names before matching, e.g. ``--rename ', int, float const\*\)$=)'`` for a
dropped trailing argument.

Every kernel that differs, renamed or not, is listed with base -> working VGPRs, SGPRs, LDS bytes, scratch bytes and
body lines: whether a change of device code costs registers, scratch or occupancy is read off that row.
"""
import argparse
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pwclonet_pylidarslam_amd import build as hip_build  # noqa: E402

CSRC = "pwclonet_pylidarslam_amd/csrc"
DEFAULT = ("fused_layers.hip", "fused_hoisted.hip", "fused_sa.hip")
_LABEL = re.compile(r"\.L(BB|func_end|func_begin|tmp)\d+")


def device_asm(tree, name, out):
    cmd = [hip_build.hipcc()] + hip_build.FLAGS + ["--cuda-device-only", "-S", os.path.join(tree, CSRC, name), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (name, r.stderr))
    with open(out) as fh:
        return fh.read()


def _clean(line):
    line = line.split(";", 1)[0].rstrip()
    return _LABEL.sub(lambda m: ".L" + m.group(1), line)


def kernels(asm):
    """{symbol: (body lines, descriptor lines)} of every kernel in one assembly file."""
    lines = asm.splitlines()
    desc, start = {}, {}
    i = 0
    while i < len(lines):
        s = lines[i].split(";", 1)[0].strip()
        if s.startswith(".amdhsa_kernel "):
            sym, block = s.split()[1], []
            i += 1
            while lines[i].strip() != ".end_amdhsa_kernel":
                block.append(_clean(lines[i]).strip())
                i += 1
            desc[sym] = block
        elif s.endswith(":") and not s.startswith("."):
            start[s[:-1]] = i
        i += 1
    out = {}
    for sym, block in desc.items():
        body, i = [], start[sym] + 1
        while not lines[i].strip().startswith(".Lfunc_end"):
            c = _clean(lines[i]).strip()
            if c:
                body.append(c)
            i += 1
        out[sym] = (body, block)
    return out


def demangled(table, renames=()):
    """The same table keyed by demangled name, after the substitutions."""
    syms = sorted(table)
    llvm = os.path.join(os.path.dirname(os.path.realpath(hip_build.hipcc())), "..", "lib", "llvm", "bin")
    exe = shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path=llvm) or shutil.which("c++filt")
    if exe is None:
        raise RuntimeError("--rename needs llvm-cxxfilt or c++filt")
    names = subprocess.run([exe] + syms, capture_output=True, text=True, check=True).stdout.splitlines()
    out = {}
    for sym, name in zip(syms, names):
        for pat, repl in renames:
            name = re.sub(pat, repl, name)
        assert name not in out, "two kernels map to " + name
        out[name] = table[sym]
    return out


_FIELDS = (("VGPR", "next_free_vgpr"), ("SGPR", "next_free_sgpr"), ("LDS", "group_segment_fixed_size"),
           ("scratch", "private_segment_fixed_size"))


def resources(kernel):
    body, block = kernel
    desc = dict(l.replace(".amdhsa_", "", 1).split(None, 1) for l in block if len(l.split(None, 1)) == 2)
    return [(label, desc.get(key, "?")) for label, key in _FIELDS] + [("lines", str(len(body)))]


def compare(name, base_tree, tmp, renames=()):
    new = kernels(device_asm(ROOT, name, os.path.join(tmp, name + ".new.s")))
    old = kernels(device_asm(base_tree, name, os.path.join(tmp, name + ".base.s")))
    if renames:
        new, old = demangled(new), demangled(old, renames)
    problems = []
    for sym in sorted(set(old) ^ set(new)):
        problems.append("%s: only in the %s tree" % (sym, "base" if sym in old else "working"))
    for sym in sorted(set(old) & set(new)):
        if old[sym][1] != new[sym][1]:
            problems.append("%s: descriptor differs" % sym)
        if old[sym][0] != new[sym][0]:
            problems.append("%s: instructions differ (%d / %d lines)" % (sym, len(old[sym][0]), len(new[sym][0])))
        if old[sym] != new[sym]:
            problems.append("        " + ", ".join("%s %s -> %s" % (k, a, b) for (k, a), (_, b) in
                                                   zip(resources(old[sym]), resources(new[sym]))))
    ninstr = sum(len(b) for b, _ in new.values())
    return name, len(new), ninstr, problems


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--base", default="HEAD~1", help="commit to compare the working tree with")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL",
                    help="substitution applied to the base tree's demangled kernel names before matching")
    ap.add_argument("sources", nargs="*", default=list(DEFAULT))
    args = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    with tempfile.TemporaryDirectory() as tmp:
        base_tree = os.path.join(tmp, "base")
        os.makedirs(base_tree)
        ar = subprocess.run(["git", "-C", ROOT, "archive", args.base, CSRC, "include"], capture_output=True, check=True)
        subprocess.run(["tar", "-x", "-C", base_tree], input=ar.stdout, check=True)
        with concurrent.futures.ThreadPoolExecutor(len(args.sources)) as ex:
            results = list(ex.map(lambda n: compare(n, base_tree, tmp, renames), args.sources))
    bad = 0
    for name, nk, ninstr, problems in results:
        print("%s: %d kernels, %d body lines: %s" % (name, nk, ninstr, "DIFFERENT from " + args.base if problems
                                                      else "identical to " + args.base))
        for p in problems:
            print("   ", p)
        bad += len(problems)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
