#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, translation unit by translation unit (no GPU needed).
usage: tools/isa_compare.py <tree before> <tree after> [--keep DIR] [tu.hip ...]

Every .hip file of chsimpy_amd/csrc (or the ones named) is compiled in both trees with the flags of
chsimpy_amd/_build.py plus `--cuda-device-only -S`.  The symbol `__hip_cuid_<hash>` -- a hash of the source text --
is replaced by a fixed string; everything else must match for "identical".  Where the whole files differ the
comparison goes on per function (split at the `_Z...:` labels, as tools/isa_stats.py does): functions only one side
has are listed, a trailing `false` template argument that the other side's name lacks is mapped away (a template
parameter that lost its second value), block labels lose their function number, and for every function whose body differs the
registers, scratch, occupancy and code bytes of both sides are printed.  --keep DIR keeps the .s files there
(DIR/before, DIR/after) and reuses the ones it finds."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

TUS = ['chs_fast_f64.hip', 'chs_fast_f32.hip', 'chs_batch.hip', 'chs_pointwise.hip', 'chs_direct.hip', 'chs_fast.hip', 'chs_api.hip',
       'chs_chirp.hip', 'chs_spectrum.hip', 'chs_morphology.hip', 'chs_components.hip', 'chs_distance.hip', 'chs_chords.hip',
       'chs_composition.hip', 'chs_two_point.hip', 'chs_contour.hip', 'chs_track.hip', 'chs_thickness.hip',
       'chs_geodesic.hip', 'chs_skeleton.hip', 'chs_transport.hip']
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-Wno-unused-value', '-Wno-unused-result', '-Wno-pass-failed',
         '-DCHS_TEST_HOOKS=1']


def assembly(tree, tu, out):
    if not os.path.exists(out):
        cmd = ['hipcc'] + FLAGS + ['-I' + os.path.join(tree, 'include'), '-I' + os.path.join(tree, 'chsimpy_amd', 'csrc'),
                                   '--cuda-device-only', '-S', os.path.join(tree, 'chsimpy_amd', 'csrc', tu), '-o', out]
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    with open(out) as fh:
        return re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', fh.read())


def functions(txt):
    """{mangled name: text of the function up to the next one} and the kernel entries of the metadata by name"""
    meta_at = txt.find('\t.amdgpu_metadata')
    code, meta = (txt[:meta_at], txt[meta_at:]) if meta_at >= 0 else (txt, '')
    parts = re.split(r'\n(_Z\w+):[^\n]*\n', code)
    # (what stands in front of a label -- .section, .globl, .type ... -- introduces the NEXT function: not part of this one)
    lead = re.compile(r'(\n\t\.(section|text|protected|globl|weak|hidden|p2align|type)\b[^\n]*|\n[ \t]*)+$')
    funcs = {n: lead.sub('', body) for n, body in zip(parts[1::2], parts[2::2])}
    entries = {}
    for e in re.split(r'\n  - ', meta)[1:]:
        m = re.search(r'\.name:\s+(\S+)', e)
        if m:
            entries[m.group(1)] = e.split('\namdhsa.target')[0]
    return funcs, entries


def demangle(names):
    out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out))


def stats(body):
    g = lambda pat: (re.search(pat, body) or [None, '?'])[1]
    return 'vgpr %s  scratch %s  occupancy %s  code %s B' % (g(r'; NumVgprs: (\d+)'), g(r'; ScratchSize: (\d+)'),
                                                             g(r'; Occupancy: (\d+)'), g(r'; codeLenInByte = (\d+)'))


def short(d):
    return re.sub(r'FCfg<([^>]*)>', lambda m: 'FCfg<' + m.group(1).replace(' ', '') + '>', d).split('(')[0]


def compare(tu, a, b, say):
    ha, hb = hashlib.sha256(a.encode()).hexdigest(), hashlib.sha256(b.encode()).hexdigest()
    fa, ma = functions(a)
    fb, mb = functions(b)
    say(f'{tu}: kernels before {len(ma)}, after {len(mb)}')
    say(f'  sha256 before {ha}\n  sha256 after  {hb}')
    if ha == hb:
        say('  identical')
        return True
    da, db = demangle(list(fa)), demangle(list(fb))
    by_name = {d: n for n, d in db.items()}
    ren, gone = {}, []
    for n, d in da.items():
        if d in by_name:
            ren[n] = by_name[d]
            continue
        d2 = re.sub(r', false>\(', '>(', d, count=1)
        if d2 in by_name:
            ren[n] = by_name[d2]
        else:
            gone.append(d)
    new = [d for n, d in db.items() if n not in ren.values()]
    renamed = sorted((n for n in ren if ren[n] != n), key=len, reverse=True)
    if renamed:
        say(f'  {len(renamed)} functions renamed (a trailing `, false` template argument dropped)')

    def norm(t, names=False):
        if names:
            for n in renamed:
                t = t.replace(n, ren[n])
        t = re.sub(r'BB\d+_', 'BB_', re.sub(r'\.L(func_end|func_begin|tmp)\d+', r'.L\1', t))
        return re.sub(r' +;', ' ;', t)   # (comments are aligned behind the labels, whose width changed)

    differ = [n for n in ren if norm(fa[n], True) != norm(fb[ren[n]])]
    meta_differ = [n for n in ren if n in ma and norm(ma[n], True) != norm(mb.get(ren[n], ''))]
    for d in gone:
        say('  only before: ' + short(d))
    for d in new:
        say('  only after:  ' + short(d))
    if not differ and not meta_differ:
        say(f'  every function both sides have is identical ({len(ren)} functions)')
    for n in differ:
        say('  differs: ' + short(da[n]))
        say('      before: ' + stats(fa[n]))
        say('      after:  ' + stats(fb[ren[n]]))
    for n in meta_differ:
        if n not in differ:
            say('  metadata differs: ' + short(da[n]))
    return not differ and not meta_differ and not gone and not new


def main():
    args = sys.argv[1:]
    keep = None
    if '--keep' in args:
        i = args.index('--keep')
        keep = args[i + 1]
        del args[i:i + 2]
    before, after = os.path.abspath(args[0]), os.path.abspath(args[1])
    tus = args[2:] or TUS
    tmp = keep or tempfile.mkdtemp(prefix='isa_compare_')
    for side in ('before', 'after'):
        os.makedirs(os.path.join(tmp, side), exist_ok=True)
    jobs = [(tree, tu, os.path.join(tmp, side, tu[:-4] + '.s')) for tu in tus for side, tree in (('before', before), ('after', after))]
    with ThreadPoolExecutor(4) as pool:
        texts = list(pool.map(lambda j: assembly(*j), jobs))
    same = True
    for k, tu in enumerate(tus):
        same = compare(tu, texts[2 * k], texts[2 * k + 1], print) and same
    if not keep:
        for _, _, f in jobs:
            os.unlink(f)
    sys.exit(0 if same else 1)


if __name__ == '__main__':
    main()
