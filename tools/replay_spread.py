"""Per-kernel duration spread over the graph replays of a rocprofv3 kernel trace, optionally against a second trace.

    python tools/replay_spread.py <kernel_trace.csv> [<other kernel_trace.csv>] [--marker adam_clip] [--skip 3] [--count 40]

Replays are delimited by the marker kernel as in tools/replay_gaps.py.  For each kernel position of the replay:
the median, minimum and maximum duration over the replays (us) and the spread max - min; with a second trace its
median, the difference of the medians, and whether that difference exceeds the first trace's spread.
"""
import csv
import statistics
import sys

from replay_gaps import short


def replays(path, marker, skip, count):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    ends = [i for i, r in enumerate(rows) if marker in r['Kernel_Name']]
    out = []
    for j in range(skip, min(skip + count, len(ends))):
        ks = rows[ends[j - 1] + 1:ends[j] + 1]
        out.append([(short(r['Kernel_Name']), (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
                    for r in ks])
    n = statistics.mode(len(s) for s in out)
    return [s for s in out if len(s) == n]


def main():
    paths = []
    for arg in sys.argv[1:]:   # the traces come before the options
        if arg.startswith('--'):
            break
        paths.append(arg)
    opt = lambda k, d: type(d)(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d   # noqa: E731
    marker, skip, count = opt('--marker', 'adam_clip'), opt('--skip', 3), opt('--count', 40)
    a = replays(paths[0], marker, skip, count)
    b = replays(paths[1], marker, skip, count) if len(paths) > 1 else None
    print('%d replays of %d kernels%s' % (len(a), len(a[0]), '' if b is None else
                                          '; other trace: %d replays of %d kernels' % (len(b), len(b[0]))))
    print('%8s %8s %8s %8s%s  kernel' % ('median', 'min', 'max', 'spread', '' if b is None else
                                        ' %8s %8s %7s' % ('other', 'delta', 'beyond')))
    tot = [0.0, 0.0]
    for k in range(len(a[0])):
        d = [s[k][1] for s in a]
        med = statistics.median(d)
        line = '%8.2f %8.2f %8.2f %8.2f' % (med, min(d), max(d), max(d) - min(d))
        tot[0] += med
        if b is not None and k < len(b[0]):
            mb = statistics.median(s[k][1] for s in b)
            tot[1] += mb
            line += ' %8.2f %8.2f %7s' % (mb, mb - med, 'yes' if abs(mb - med) > max(d) - min(d) else 'no')
        print(line + '  ' + a[0][k][0] + ('' if b is None or b[0][k][0] == a[0][k][0] else '  ->  ' + b[0][k][0]))
    print('sum of medians: %.2f%s' % (tot[0], '' if b is None else '; other %.2f (%.2f)' % (tot[1], tot[1] - tot[0])))


if __name__ == '__main__':
    main()
