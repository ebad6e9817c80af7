#!/usr/bin/env python3
"""Per-kernel statistics from the database a `rocprofv3 --kernel-trace --stats -d DIR -o NAME -- <command>` run leaves
(DIR/NAME_results.db, the rocpd format): one CSV row per (kernel, grid) - the launches of one kernel at different shapes
stay apart, which the profiler's own per-kernel summary does not do - with the workgroups of the launch, the calls, the
mean and the total time in microseconds, by total time.  `--like` keeps the kernels whose name contains one of the given
substrings.

Usage: python tools/rocpd_kernel_stats.py DIR/NAME_results.db OUT.csv [--like cspfit headfit csp_head]"""
import argparse
import sqlite3

ap = argparse.ArgumentParser()
ap.add_argument("db")
ap.add_argument("out")
ap.add_argument("--like", nargs="*", default=[])
args = ap.parse_args()

con = sqlite3.connect(args.db)
where = " or ".join("name like ?" for _ in args.like) or "1"
rows = con.execute("select name, grid_x / workgroup_x, count(*), avg(end - start) / 1e3, sum(end - start) / 1e3 from kernels "
                   f"where {where} group by name, grid_x order by 5 desc", [f"%{s}%" for s in args.like]).fetchall()
with open(args.out, "w") as f:
    f.write("kernel,workgroups,calls,avg_us,total_us\n")
    for name, wg, calls, avg, total in rows:
        f.write('"%s",%d,%d,%.1f,%.1f\n' % (name.replace("range_hip::", ""), wg, calls, avg, total))
print(f"{args.out}: {len(rows)} rows")
