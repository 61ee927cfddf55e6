"""Developer tool: registers, scratch and occupancy of the kernels of one translation unit of the library, or of all
of them, from hipcc -Rpass-analysis=kernel-resource-usage (device-only compile, no GPU needed).

    python tools/kernel_resources.py [name-filter ...]                     (the core unit, ndlqr_hip.hip)
    python tools/kernel_resources.py --unit hip_box.hip [name-filter ...]  (another unit of rslqr_amd/build.py)
    python tools/kernel_resources.py --instance 12 4 [name-filter ...]     (small_instance.hip for one block size)
    python tools/kernel_resources.py --reduced 4 [name-filter ...]         (reduced_instance.hip for one tile count)
    python tools/kernel_resources.py --all                                 (every unit and instance: one sorted table
                                                                            with full kernel names; a kernel that shows
                                                                            twice is compiled into two units)
"""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def resources(src, extra, width=58):
    """One line per kernel of the unit `src` (a file of rslqr_amd/csrc) compiled with the flags `extra`."""
    csrc = os.path.join(ROOT, "rslqr_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=off", "-fPIC",
               "--cuda-device-only"] + extra + ["-I" + os.path.join(ROOT, "include"), "-I" + csrc,
               "-c", os.path.join(csrc, src), "-o", os.path.join(tmp, "dev.o"), "-Rpass-analysis=kernel-resource-usage"]
        txt = subprocess.run(cmd, stderr=subprocess.PIPE, text=True).stderr
    filt = subprocess.run(["c++filt"], input=txt, stdout=subprocess.PIPE, text=True).stdout
    rows = []
    for blk in re.split(r"remark: [^\n]*Function Name: ", filt)[1:]:
        name = blk.split("\n")[0].split("(")[0].replace("void ndlqr::", "").replace("ndlqr::", "")
        g = lambda k: re.search(k + r": (\S+)", blk).group(1)  # noqa: E731
        rows.append((name, "%-*s VGPR %3s AGPR %3s scratch %4s occ %s LDS %s" % (
            width, name[:width] if width else name, g("VGPRs"), g("AGPRs"), g(r"ScratchSize \[bytes/lane\]"),
            g(r"Occupancy \[waves/SIMD\]"), g(r"LDS Size \[bytes/block\]"))))
    return rows


def table(units):
    """The sorted table of the (src, extra) units, full kernel names."""
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(os.cpu_count() or 2, 16)) as pool:
        parts = list(pool.map(lambda u: resources(u[0], u[1], width=0), units))
    return sorted(line for part in parts for _, line in part)


def main():
    args = sys.argv[1:]
    if "--all" in args:
        import rslqr_amd.build as b
        print("\n".join(table([(src, extra) for _, src, extra, _ in b.hip_jobs()])))
        return
    extra, src = [], "ndlqr_hip.hip"
    if args[:1] == ["--unit"]:
        src, args = args[1], args[2:]
    elif args[:1] == ["--instance"]:
        extra, src, args = ["-DNDLQR_INST_NX=" + args[1], "-DNDLQR_INST_NU=" + args[2]], "small_instance.hip", args[3:]
    elif args[:1] == ["--reduced"]:
        extra, src, args = ["-DNDLQR_RED_NB=" + args[1]], "reduced_instance.hip", args[2:]
    filters = [a for a in args if not a.startswith("-")] or [""]
    for name, line in resources(src, extra):
        if any(f in name for f in filters):
            print(line)


if __name__ == "__main__":
    main()
