"""Two step logs of the same solve from two builds (UVS_DEBUG_LIN_TIMELINE, see tools/lin_timeline.py), interval by interval: the cycles between consecutive stamps of a wave,
summed over one LM iteration by (stamp, next stamp) pair, build A against build B.  The two logs must walk the same stamp sequence (same window, same LM path).
usage: python tools/lin_timeline_diff.py <file A> <file B> [linearization index, default 2] [waves, default 0,4: the first evaluator and the first gatherer of the 512-thread build]"""
import collections, os, re, subprocess, sys
HERE = os.path.dirname(os.path.abspath(__file__))
which = sys.argv[3] if len(sys.argv) > 3 else "2"
show = [int(x) for x in (sys.argv[4] if len(sys.argv) > 4 else "0,4").split(",")]


def parse(path):
    out = subprocess.run([sys.executable, os.path.join(HERE, "lin_timeline.py"), path, which], capture_output=True, text=True, check=True).stdout.splitlines()
    waves = {}
    for l in out:
        m = re.match(r"wave (\d): (.*)", l)
        if m: waves[int(m.group(1))] = [(t.split("@")[0], int(t.split("@")[1])) for t in m.group(2).split()]
    return out[0], waves


ha, a = parse(sys.argv[1]); hb, b = parse(sys.argv[2])
print("A:", ha); print("B:", hb)
for w in show:
    if w not in a or w not in b: continue
    sa, sb = a[w], b[w]
    if [x[0] for x in sa] != [x[0] for x in sb]:
        print("wave %d: the stamp sequences differ (%d and %d stamps)" % (w, len(sa), len(sb))); continue
    agg = collections.OrderedDict()
    for i in range(len(sa) - 1):
        d = agg.setdefault(sa[i][0] + " -> " + sa[i + 1][0], [0, 0, 0])
        d[0] += 1; d[1] += sa[i + 1][1] - sa[i][1]; d[2] += sb[i + 1][1] - sb[i][1]
    print("wave %d: interval (times per iteration)            A          B      B - A" % w)
    for k, (n, x, y) in agg.items():
        print("   %-28s x%-3d %10d %10d %8d" % (k, n, x, y, y - x))
