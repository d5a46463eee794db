#!/usr/bin/env python3
"""Device code of a parent revision against the working tree, kernel by kernel — the proof a refactor of the device headers owes.

    python tools/listing_diff.py <parent-rev> [--unit NAME ...] [--user-units] [--jobs N] [--rename OLD=NEW ...] [--show]

For every kernel unit of build.py (UNITS minus HOST_ONLY_UNITS; --unit picks some) the device listing is made the way the first step
of build.compile_via_listing makes it (FLAGS, the fixed -cuid, --cuda-device-only -S), once from a `git worktree` of <parent-rev>
under a temporary directory and once from the working tree.  --user-units adds two run-time units (a source of examples/ pasted into
rtgr_user_unit.hip.in by each tree's own user_metric.py: its paste_source, FLAGS and unit_defines): SCHWARZSCHILD_ISOTROPIC declared
stationary, and the objects of SHAPES_WITH_REACH for Kerr–Schild as written, a = 0.  A unit that only one side has counts as differing.
Kernels are paired by symbol; --rename 'lc_sum_kernel<double>=reduce_sum_kernel<rtgr::LcModel<double>>' pairs a parent's kernel with its
successor of another name (the names the table prints), and --show lists, for a pair whose histograms differ, the opcodes that do.

Printed per kernel (the table of profiles/grid/refactor_isa.md): instruction count, whether the opcode histogram is the same — whole
histograms are compared, no opcode is singled out —, vgpr / sgpr / agpr / scratch / LDS from the code object metadata, and whether the
kernel's text is byte-identical; then the sha256 of every listing (first 16 digits, as in profiles/host_twins/README.md).  Exit status 0
when every listing is byte-identical, 1 otherwise.  Needs hipcc, no GPU; at most 16 compiler processes."""
import argparse
import collections
import concurrent.futures
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (examples module, source, arguments of user_metric.unit_defines; built_for is (metric kind by name, generic, spin))
USER_UNITS = {"unit_metric_stationary": ("user_metrics", "SCHWARZSCHILD_ISOTROPIC", {"stationary": True}),
              "unit_objects_ksref": ("user_objects", "SHAPES_WITH_REACH", {"built_for": ("KS_REF", False, False)})}
RESOURCES = [("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("agpr", ".agpr_count"), ("scratch", ".private_segment_fixed_size"),
             ("lds", ".group_segment_fixed_size")]


def _module(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _user_metric(tree):
    """<tree>/raytracegr.jl_amd/user_metric.py, imported as part of a package whose __init__ is NOT run (it would load the built library)"""
    name = "rtgr_ld_" + hashlib.sha256(tree.encode()).hexdigest()[:8]
    pkg = types.ModuleType(name)
    pkg.__path__ = [os.path.join(tree, "raytracegr.jl_amd")]
    sys.modules[name] = pkg
    return importlib.import_module(name + ".user_metric")


def jobs_of(tree, out_dir, units, user_units):
    """[(name, command, listing path)] for one source tree; unit lists, flags and a run-time unit's defines are that tree's own"""
    um = _user_metric(tree)
    b, csrc = um._build, um.CSRC
    jobs = []
    for u in b.UNITS:
        name = os.path.splitext(u)[0]
        if u in b.HOST_ONLY_UNITS or (units and name not in units):
            continue
        cuid = "-cuid=" + hashlib.sha256(u.encode()).hexdigest()[:16]
        asm = os.path.join(out_dir, name + ".s")
        jobs.append((name, [b.HIPCC] + b.FLAGS + [cuid, "--cuda-device-only", "-S", "-o", asm, os.path.join(csrc, u)], asm))
    for name, (mod, var, how) in (USER_UNITS.items() if user_units else ()):
        source = getattr(_module(os.path.join(tree, "examples", mod + ".py"), "rtgr_ex_" + mod), var)
        if "built_for" in how:
            how = {"built_for": (getattr(um._abi, how["built_for"][0]),) + how["built_for"][1:]}
        defs, _ = um.unit_defines(source, **how)
        src, asm = os.path.join(out_dir, name + ".hip"), os.path.join(out_dir, name + ".s")
        with open(src, "w") as fh:
            fh.write(um.paste_source(open(um.TEMPLATE).read(), source))
        # (a fixed -cuid — hipcc's own hashes the path and the text, the template's #include lines among it — and no -DRTGR_HEADER_HASH,
        #  which differs between the two sides by design)
        cuid = "-cuid=" + hashlib.sha256(name.encode()).hexdigest()[:16]
        jobs.append((name, [b.HIPCC] + um.FLAGS + defs + [cuid, "-S", "-I", csrc, "-o", asm, src], asm))
    return jobs


def run_jobs(jobs, workers):
    def one(job):
        name, cmd, _ = job
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{name}: {' '.join(cmd)}\n{r.stderr[-4000:]}")
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as ex:
        list(ex.map(one, jobs))


def kernels_of(listing):
    """{kernel symbol: (text of its body, instruction count, opcode histogram, {resource: value})}, in listing order"""
    lines = listing.split("\n")
    meta, cur = {}, None
    for l in lines[next((i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")), len(lines)):]:
        if l.startswith("  - "):
            cur = {}
            l = "    " + l[4:]
        m = re.match(r"^    (\.\w+):\s*(\S+)\s*$", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == ".name":
                meta[m.group(2)] = cur
    out = {}
    for start, l in enumerate(lines):
        name = l.split(";")[0].rstrip()[:-1]
        if l[:1] in ("\t", " ", ".") or not l.split(";")[0].rstrip().endswith(":") or name not in meta:
            continue
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = lines[start:end]
        ops = [b.split()[0] for b in body if b.startswith("\t") and not b.lstrip().startswith((".", ";"))]
        out[name] = ("\n".join(body), len(ops), collections.Counter(ops), {k: meta[name].get(f, "?") for k, f in RESOURCES})
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True)
        return dict(zip(names, (re.sub(r"^void rtgr::|\(.*$", "", d) for d in r.stdout.split("\n"))))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def compare(parent_dir, branch_dir, names, renames=(), show=False):
    """prints the table and the hashes; names: {unit: which sides have it}; renames: [(parent kernel, branch kernel)] by the names the
    table prints, spaces ignored — the pair is compared with the branch's symbol read as the parent's; -> number of listings that are
    not byte-identical on both sides"""
    renames = {o.replace(" ", ""): n.replace(" ", "") for o, n in renames}
    print("| unit | kernel | instructions parent / branch | opcode histogram | vgpr | sgpr | agpr | scratch | lds | listing |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    hashes, differing = [], 0
    for name, sides in names.items():
        if len(sides) < 2:
            print(f"| {name} | only in the {sides[0]} | | | | | | | | |")
            hashes.append((name,) + (("—", "—")))
            differing += 1
            continue
        pt, bt = (open(os.path.join(d, name + ".s")).read() for d in (parent_dir, branch_dir))
        pt, bt = pt.replace(parent_dir, "<dir>"), bt.replace(branch_dir, "<dir>")      # (a run-time unit's listing names its pasted source file)
        hashes.append((name, hashlib.sha256(pt.encode()).hexdigest()[:16], hashlib.sha256(bt.encode()).hexdigest()[:16]))
        differing += pt != bt
        pk, bk = kernels_of(pt), kernels_of(bt)
        pretty = demangle(list(pk) + [k for k in bk if k not in pk])
        bare = {k: v.replace(" ", "") for k, v in pretty.items()}
        heir = {k: next((b for b in bk if b not in pk and bare[b] == renames.get(bare[k])), None) for k in pk if k not in bk}
        for k in list(pk) + [k for k in bk if k not in pk and k not in heir.values()]:
            if k in heir and heir[k]:
                b = heir[k]
                bk[k] = (bk[b][0].replace(b, k),) + bk[b][1:]
                pretty[k] += "` -> `" + pretty[b]
            if k not in pk or k not in bk:
                print(f"| {name} | `{pretty[k]}` | {'only in the ' + ('parent' if k in pk else 'branch')} | | | | | | | |")
                continue
            (ptxt, pn, ph, pr), (btxt, bn, bh, br) = pk[k], bk[k]
            same = "byte-identical" if ptxt == btxt else ("schedule differs" if ph == bh else "DIFFERS")
            print(f"| {name} | `{pretty[k]}` | {pn} / {bn} | {'identical' if ph == bh else 'DIFFERS'} | "
                  + " | ".join(f"{pr[r]} / {br[r]}" for r, _ in RESOURCES) + f" | {same} |")
            if show and ph != bh:
                print("|  |  | " + ", ".join(f"{op} {ph[op]} / {bh[op]}" for op in sorted(set(ph) | set(bh)) if ph[op] != bh[op]) + " | | | | | | | |")
    print("\n| unit | parent | branch | whole listing |\n|---|---|---|---|")
    for name, p, b in hashes:
        print(f"| `{name}` | `{p}` | `{b}` | {'byte-identical' if p == b and p != '—' else 'differs'} |")
    return differing


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("--unit", action="append", default=[], help="unit name without .hip (repeatable); default: every kernel unit")
    ap.add_argument("--user-units", action="store_true", help="also two run-time units built from examples/")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 4))
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="pair the parent's kernel OLD with the branch's NEW (the names the table prints; repeatable)")
    ap.add_argument("--show", action="store_true", help="for a pair whose histograms differ, print the opcodes that do (parent / branch)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="rtgr_listing_diff_") as tmp:
        tree, pdir, bdir = (os.path.join(tmp, d) for d in ("parent", "listings_parent", "listings_branch"))
        subprocess.check_call(["git", "-C", ROOT, "worktree", "add", "--detach", "--quiet", tree, a.parent])
        try:
            os.makedirs(pdir)
            os.makedirs(bdir)
            pj, bj = jobs_of(tree, pdir, a.unit, a.user_units), jobs_of(ROOT, bdir, a.unit, a.user_units)
            names = {}
            for side, jobs in (("parent", pj), ("branch", bj)):
                for n, _, _ in jobs:
                    names.setdefault(n, []).append(side)
            run_jobs(pj + bj, max(1, min(16, a.jobs)))
            differing = compare(pdir, bdir, names, [r.split("=", 1) for r in a.rename], a.show)
        finally:
            subprocess.call(["git", "-C", ROOT, "worktree", "remove", "--force", tree])
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
