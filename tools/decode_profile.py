"""Measurement record of the batched beam search: writes profiles/decode_batch.json.

  1. tools/bench_decode.py --batch 1,8: the one-utterance path and the batched path, alternately, in one process;
  2. rocprofv3 --kernel-trace --stats over two batched calls (a run of its own);
  3. rocprofv3 --memory-copy-trace over the same, both at two decode lengths (a run each): the copies of a batch must not
     grow with the number of decode steps.
Every child runs under its own time limit and the first failure stops the script.
Usage: python tools/decode_profile.py [--out profiles/decode_batch.json] [--work /tmp/decode_profile]"""
import argparse, csv, glob, json, os, re, subprocess, sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
BENCH = [sys.executable, os.path.join(ROOT, 'tools', 'bench_decode.py')]


def run(cmd, limit):
    r = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f'{cmd[:6]} ... exited with {r.returncode}; stopping')
    return r.stdout


def last_json(txt):
    return json.loads([l for l in txt.splitlines() if l.startswith('{')][-1])


def find(d, suffix):
    f = glob.glob(os.path.join(d, '**', '*' + suffix), recursive=True)
    if not f:
        raise SystemExit(f'no *{suffix} under {d}')
    return f[0]


def short(name):
    m = re.match(r'(?:void )?(?:\(anonymous namespace\)::)?([\w:]+)', name)
    return (m.group(1) if m else name)[:60]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'decode_batch.json'))
    ap.add_argument('--work', default='/tmp/decode_profile')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--utts', type=int, default=8)
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    bench = last_json(run(BENCH + ['--batch', '1,8', '--rounds', str(a.rounds), '--utts', str(a.utts)], 600))
    one, b1, b8 = bench['one_utterance_path'], bench['batched']['U=1'], bench['batched']['U=8']
    width = lambda r: r['spread_s_per_utt'][1] - r['spread_s_per_utt'][0]
    acc = {
        'U=1 not slower than the one-utterance path by more than the spread':
            bool(b1['gpu_s_per_utt'] - one['gpu_s_per_utt'] <= max(width(one), width(b1))),
        'U=8 utterances/s above the one-utterance path by more than the spread':
            bool(one['gpu_s_per_utt'] - b8['gpu_s_per_utt'] > max(width(one), width(b8))),
    }
    prof = ['--batch', '8', '--only-batch', '2', '--utts', '8']
    kernels, copies, blits, d2h = None, {}, {}, []
    for ratio in ('0.1', '0.05'):
        kd = os.path.join(a.work, 'kernels_' + ratio)
        info = last_json(run(['rocprofv3', '--kernel-trace', '--stats', '-d', kd, '-o', 'k', '--output-format', 'csv', '--'] + BENCH + prof +
                             ['--ratio', ratio], 400))
        rows = list(csv.DictReader(open(find(kd, 'kernel_stats.csv'))))
        rows.sort(key=lambda r: -float(r['TotalDurationNs']))
        label = f'{info["decode_steps"]} decode steps'
        # the runtime stages a pageable copy through a blit kernel: those show up here, not in the memory-copy trace
        blits[label] = sum(int(r['Calls']) for r in rows if 'copyBuffer' in r['Name'])
        if kernels is None:
            steps_full = info['decode_steps']
            kernels = [dict(kernel=short(r['Name']), calls=int(r['Calls']), total_us=float(r['TotalDurationNs']) / 1e3,
                            avg_us=float(r['AverageNs']) / 1e3, percent=float(r['Percentage'])) for r in rows[:24]]
        md = os.path.join(a.work, 'copies_' + ratio)
        run(['rocprofv3', '--memory-copy-trace', '-d', md, '-o', 'm', '--output-format', 'csv', '--'] + BENCH + prof + ['--ratio', ratio], 400)
        n = {}
        for r in csv.DictReader(open(find(md, 'memory_copy_trace.csv'))):
            n[r['Direction']] = n.get(r['Direction'], 0) + 1
        copies[label] = n
        d2h.append(sum(v for k, v in n.items() if k.endswith('TO_HOST')) + blits[label])
    out = dict(bench, acceptance=acc,
               kernel_stats=dict(run=f'rocprofv3 --kernel-trace --stats, process of its own: model set-up, then 3 batched calls of U=8 '
                                     f'({steps_full} decode steps each; 1 warm-up + 2)', top=kernels),
               memory_copies=dict(run='rocprofv3 --memory-copy-trace and, separately, --kernel-trace --stats, a process each per decode '
                                      'length: model set-up, then 3 batched calls of U=8 (two device loops of 4 utterances each); traced '
                                      'copies counted by direction over the whole process, plus the dispatches of the runtime\'s blit '
                                      'kernel (__amd_rocclr_copyBuffer), which carries the pageable copies the copy trace does not list',
                                  traced_copies_by_decode_length=copies, blit_kernel_dispatches_by_decode_length=blits,
                                  copies_toward_host_upper_bound=d2h,
                                  independent_of_decode_steps=bool(len(set(d2h)) == 1)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, 'w'), indent=1)
    print(json.dumps(dict(acceptance=acc, one=one['gpu_s_per_utt'], b1=b1['gpu_s_per_utt'], b8=b8['gpu_s_per_utt'], d2h=d2h)))


if __name__ == '__main__':
    main()
