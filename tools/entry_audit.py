"""Entry audit of kernels in a gfx950 assembly listing: what a wave executes in front of its first vector memory load.

    hipcc --offload-arch=gfx950 <the product's flags, prima_cpp_amd/build.py> --cuda-device-only -S \\
          -Rpass-analysis=kernel-resource-usage prima_cpp_amd/csrc/mmvq.hip -o mmvq.s 2> mmvq.remarks
    python tools/entry_audit.py mmvq.s [--remarks mmvq.remarks] [--match gemv_q_kernel] [--hot]

Per kernel: static instruction lines in front of the first global / buffer / flat load and in front of the first non-temporal one (the mat-vec's
weight loads; the backward-compatibility trampoline of the kernarg preload - the loads that fill the preloaded SGPRs on firmware that does not,
their wait and the branch over the padding - is counted separately), how many scalar-cache waits (s_waitcnt lgkmcnt) sit there, how many scalar
loads were issued there, and - with --remarks - VGPRs, SGPRs and scratch bytes. Static counts: a scalar branch in front of the load counts
both sides."""
import argparse
import re
import subprocess
import sys


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
            return r.stdout.splitlines()
        except (OSError, subprocess.CalledProcessError):
            continue
    return list(names)


def kernels(path):
    """yields (symbol, [instruction lines])"""
    sym, body, types = None, [], set()
    lines = open(path).read().splitlines()
    for ln in lines:
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m:
            types.add(m.group(1))
    for ln in lines:
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", ln)
        if m and m.group(1) in types:
            if sym:
                yield sym, body
            sym, body = m.group(1), []
            continue
        if sym is None:
            continue
        s = ln.strip()
        if s.startswith(".Lfunc_end"):
            yield sym, body
            sym, body = None, []
            continue
        if not s or s.startswith((".", ";", "//")) or re.match(r"^[\w.$]+:", s):
            continue
        body.append(s.split(";")[0].strip())
    if sym:
        yield sym, body


def audit(body):
    """(trampoline lines, then for the first vector load and for the first non-temporal - weight - load: (lines, scalar-cache waits, scalar loads) in front)"""
    tramp = 0
    head = body[:8]
    if head and head[0].startswith("s_load_") and any(b.startswith("s_branch") for b in head):
        # trampoline: s_load of the preloaded arguments, their wait, a branch over the padding
        tramp = next(i for i, b in enumerate(head) if b.startswith("s_branch")) + 1
    out = []
    for is_target in (lambda ins: re.match(r"^(global_load|buffer_load|flat_load|scratch_load)", ins),
                      lambda ins: re.match(r"^(global_load|buffer_load|flat_load)", ins) and re.search(r"\bnt\b", ins)):
        n = waits = sloads = 0
        found = False
        for ins in body[tramp:]:
            if is_target(ins):
                found = True
                break
            n += 1
            if ins.startswith("s_waitcnt") and "lgkmcnt" in ins:
                waits += 1
            if ins.startswith("s_load_"):
                sloads += 1
        out.append((n, waits, sloads) if found else (-1, -1, -1))
    return tramp, out[0], out[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--remarks")
    ap.add_argument("--match", default="")
    a = ap.parse_args()
    res = {}
    if a.remarks:
        cur = None
        for ln in open(a.remarks):
            m = re.search(r"Function Name: (\S+)", ln)
            if m:
                cur = res.setdefault(m.group(1), {})
            for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                             ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
                m = re.search(pat, ln)
                if m and cur is not None:
                    cur[key] = int(m.group(1))
    ks = list(kernels(a.asm))
    names = demangle([k for k, _ in ks])
    print("first vector load (activation) | first non-temporal load (weights): static lines / scalar-cache waits / scalar loads in front, trampoline apart")
    print(f"{'lines':>6s} {'waits':>5s} {'s_load':>6s} | {'lines':>6s} {'waits':>5s} {'s_load':>6s} {'tramp':>5s} {'vgpr':>5s} {'sgpr':>5s} {'scratch':>7s}  kernel")
    for (sym, body), name in zip(ks, names):
        if a.match and a.match not in name:
            continue
        tramp, f, w = audit(body)
        r = res.get(sym, {})
        short = re.sub(r"^void \(anonymous namespace\)::", "", name)
        short = re.sub(r"\(.*$", "", short)
        print(f"{f[0]:6d} {f[1]:5d} {f[2]:6d} | {w[0]:6d} {w[1]:5d} {w[2]:6d} {tramp:5d} {r.get('vgpr', -1):5d} {r.get('sgpr', -1):5d} {r.get('scratch', -1):7d}  {short}")


if __name__ == "__main__":
    sys.exit(main())
