"""Summary of a rocprofv3 kernel trace of tools/node_solver_probe.py with direct nodes: per contour sweep (a sweep ends with
k_node_finish) the direct part -- factorisation kernels (k_lu_*, k_mf_extend_add, ...) and substitution kernels (k_solve_*,
k_mf_fwd_*, k_mf_bwd_*, k_mf_scatter) -- against the Krylov part (k_spmm_row, k_fused_*): wall span from first start to last
end, time with a kernel running, launches.  The difference of span and busy time is what the device waits for the host.

  python tools/node_solver_trace.py <kernel_trace.csv> [direct nodes per sweep]"""
import csv
import sys

import numpy as np

SUBST = ("k_solve_", "k_mf_fwd", "k_mf_bwd", "k_mf_scatter")
KRYLOV = ("k_spmm", "k_fused", "k_cocg")
FACTOR = ("k_lu_", "k_mf_extend", "k_mf_assemble", "k_mf_form", "k_mf_check", "k_mf_zero")


def part(name):
    n = name.replace("void ", "")
    for tag, keys in (("substitution", SUBST), ("krylov", KRYLOV), ("factor", FACTOR)):
        if n.startswith(keys):
            return tag
    return "other"


def main():
    rows = [r for r in csv.DictReader(open(sys.argv[1])) if r["Kind"] == "KERNEL_DISPATCH"]
    nd = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    sweeps, cur = [], []
    for r in rows:
        cur.append(r)
        if "k_node_finish" in r["Kernel_Name"]:
            sweeps.append(cur)
            cur = []
    print("%d sweeps with direct nodes; times in ms" % len(sweeps))
    print("%5s | %28s | %28s | %28s" % ("sweep", "factor: span busy launches", "substitution: span busy launches", "krylov: span busy launches"))
    acc = {"substitution": [], "krylov": [], "factor": []}
    for i, sw in enumerate(sweeps):
        line = "%5d" % i
        for tag in ("factor", "substitution", "krylov"):
            ks = [r for r in sw if part(r["Kernel_Name"]) == tag]
            if not ks:
                line += " | %28s" % "-"
                continue
            t0, t1 = min(int(r["Start_Timestamp"]) for r in ks), max(int(r["End_Timestamp"]) for r in ks)
            busy = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in ks)
            acc[tag].append(((t1 - t0) * 1e-6, busy * 1e-6, len(ks)))
            line += " | %9.2f %9.2f %8d" % ((t1 - t0) * 1e-6, busy * 1e-6, len(ks))
        print(line)
    for tag, v in acc.items():
        if v:
            a = np.array(v)
            print("%-12s median span %.2f ms, busy %.2f ms, %d launches per sweep (%d sweeps)" % (tag, np.median(a[:, 0]), np.median(a[:, 1]),
                                                                                               int(np.median(a[:, 2])), len(v)))
    s = np.array(acc["substitution"])
    print("substitution per direct node and sweep: span %.2f ms, busy %.2f ms (%d direct nodes)" % (np.median(s[:, 0]) / nd, np.median(s[:, 1]) / nd, nd))


if __name__ == "__main__":
    main()
