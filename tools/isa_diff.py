#!/usr/bin/env python3
"""Is the device code of this tree the device code of <git rev>?  No GPU needed.

    python tools/isa_diff.py <git rev> [-j N]

Exports csrc/ and include/ of <rev> with `git archive` into a temporary directory, runs `make asm` there and here (every source with
its own Makefile flags, the mutant sources also with the two mutant masks), cuts each .s into its kernels and compares them with
local labels renumbered and comments stripped.  One line per kernel: same / DIFF / only in <rev> / only here.  A kernel missing from
the same-named .s of the other tree but present under the same symbol in exactly one other .s there is compared with that one and
printed with both file names, marked (moved).  Exit status 1 on any DIFF or `only in <rev>` (a kernel that only exists here is new
code, not changed code).  A revision whose Makefile has no asm target
is given this tree's csrc/asm.mk next to its own Makefile, so each side is compiled with its own flags.
"""
import argparse
import pathlib
import re
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = next(ROOT.glob("*_amd/csrc"))
REL = CSRC.relative_to(ROOT)


def make_asm(csrc, jobs):
    mk = ["make", "-C", str(csrc), f"-j{jobs}", "-f", "Makefile"]
    if not (csrc / "asm.mk").exists():
        mk += ["-f", str(CSRC / "asm.mk")]
    subprocess.run(mk + ["asm"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)


def kernels(path):
    """{kernel symbol: normalised body} of one .s file (.amdhsa_kernel names the kernels; a body runs from `sym:` to .Lfunc_end)"""
    text = path.read_text()
    out = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        body = re.search(rf"^{re.escape(sym)}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S).group(1)
        labels = {}
        lines = []
        for line in body.splitlines():
            line = line.split(";")[0].rstrip()
            line = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), line)
            if line:
                lines.append(line)
        out[sym] = "\n".join(lines)
    return out


def compare(asm_rev, asm_here, rev, out=sys.stdout):
    """prints the verdict lines for build/asm of the two trees; True when nothing differs and nothing of <rev> is missing"""
    ok = True
    files = sorted({p.relative_to(d) for d in (asm_rev, asm_here) for p in d.rglob("*.s")})
    a_all = {rel: kernels(asm_rev / rel) if (asm_rev / rel).exists() else {} for rel in files}
    b_all = {rel: kernels(asm_here / rel) if (asm_here / rel).exists() else {} for rel in files}
    moved = {}                                  # (file here, symbol) -> file of <rev>: the symbol left its file for exactly one other
    for rel in files:
        for sym in a_all[rel].keys() - b_all[rel].keys():
            homes = [r for r in files if sym in b_all[r]]
            if len(homes) == 1:
                moved[(homes[0], sym)] = rel
    home_of = {(rel, sym): home for (home, sym), rel in moved.items()}
    for rel in files:
        a, b = a_all[rel], b_all[rel]
        for sym in sorted(a.keys() | b.keys()):
            if (rel, sym) in moved and sym not in a:
                continue                        # printed with the file it came from
            if (rel, sym) in home_of:
                home = home_of[(rel, sym)]
                verdict = "same" if a[sym] == b_all[home][sym] else "DIFF"
                where = f"{rel} -> {home} (moved)"
            else:
                verdict = f"only in {rev}" if sym not in b else "only here" if sym not in a else "same" if a[sym] == b[sym] else "DIFF"
                where = str(rel)
            ok &= verdict in ("same", "only here")
            print(f"{verdict:<8}  {where}  {sym}", file=out)
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("rev")
    ap.add_argument("-j", type=int, default=8)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        archive = subprocess.run(["git", "-C", str(ROOT), "archive", args.rev, str(REL), "include"], check=True, stdout=subprocess.PIPE)
        subprocess.run(["tar", "-x", "-C", tmp], input=archive.stdout, check=True)
        make_asm(pathlib.Path(tmp) / REL, args.j)
        make_asm(CSRC, args.j)
        ok = compare(pathlib.Path(tmp) / REL / "build/asm", CSRC / "build/asm", args.rev)
    print("identical" if ok else "NOT identical")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
