"""per-kernel mean duration and mean gap before it over all steady-state launches of a rocprofv3 kernel trace"""
import sys, sqlite3, csv, collections
db, out = sys.argv[1], sys.argv[2]
cur = sqlite3.connect(db).cursor()
rows = cur.execute("select name, start, end from kernels order by start").fetchall()
dur, gap = collections.defaultdict(list), collections.defaultdict(list)
for i in range(1, len(rows)):
    n = rows[i][0].split('(')[0][-60:]
    g = (rows[i][1] - rows[i - 1][2]) / 1e3
    dur[n].append((rows[i][2] - rows[i][1]) / 1e3)
    if g < 20.0:          # (longer: the host was late, not the device)
        gap[n].append(g)
with open(out, 'w', newline='') as f:
    w = csv.writer(f)
    w.writerow(['kernel', 'calls', 'mean_duration_us', 'median_duration_us', 'mean_gap_before_us', 'median_gap_before_us', 'gaps_counted'])
    for n in sorted(dur, key=lambda k: -sum(dur[k])):
        if len(dur[n]) < 100:
            continue
        d, g = sorted(dur[n]), sorted(gap[n]) or [0.0]
        w.writerow([n, len(d), round(sum(d) / len(d), 3), round(d[len(d) // 2], 3), round(sum(g) / len(g), 3), round(g[len(g) // 2], 3), len(gap[n])])
print(open(out).read())
