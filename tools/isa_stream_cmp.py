#!/usr/bin/env python3
"""isa_cmp.py PARENT_DIR NEW_DIR: per kernel (matched by name) compare
(a) the stream of v_mfma / ds_ / global_ / buffer_ / scratch_ / s_barrier / s_waitcnt / s_sleep / s_cbranch / s_branch / s_endpgm lines with operands
(b) .vgpr_count .agpr_count .sgpr_count .vgpr_spill_count .sgpr_spill_count .private_segment_fixed_size .group_segment_fixed_size"""
import re, sys, difflib
PAT = re.compile(r'^\s*(v_mfma|ds_|global_|buffer_|scratch_|s_barrier|s_waitcnt|s_sleep|s_cbranch|s_branch|s_endpgm)')
META = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.vgpr_spill_count', '.sgpr_spill_count', '.private_segment_fixed_size', '.group_segment_fixed_size')
def parse(path):
    streams, meta, cur = {}, {}, None
    lines = open(path).read().split('\n')
    for ln in lines:
        m = re.match(r'^(_Z\w+):', ln)
        if m: cur = m.group(1); streams[cur] = []; continue
        if ln.startswith('.Lfunc_end'): cur = None; continue
        if cur and PAT.match(ln): streams[cur].append(re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r'\s*;.*$', '', ln.strip())))   # labels: drop the function's index in the file
    # metadata: YAML list items under amdhsa.kernels
    block = {}
    for ln in lines:
        m = re.match(r'^\s*(?:-\s+)?(\.[a-z_]+):\s*(\S+)\s*$', ln)
        if not m: continue
        k, v = m.groups()
        if k in META: block[k] = v
        elif k == '.name' and v.startswith('_Z') : block['.name'] = v
        elif k == '.wavefront_size':
            if '.name' in block: meta[block['.name']] = {q: block.get(q) for q in META}
            block = {}
    return streams, meta
bad = 0
for f in ('conv_win', 'conv_win16', 'conv_win2'):
    sa, ma = parse(f'{sys.argv[1]}/{f}.s'); sb, mb = parse(f'{sys.argv[2]}/{f}.s')
    print(f'== {f}.hip: kernels {len(sa)} / {len(sb)}, metadata records {len(ma)} / {len(mb)}, names equal: {sorted(sa) == sorted(sb) and sorted(ma) == sorted(mb) and sorted(sa) == sorted(ma)}')
    if sorted(sa) != sorted(sb): bad += 1
    ns = nm = 0
    for k in sorted(sa):
        if k not in sb: continue
        if sa[k] != sb[k]:
            ns += 1
            d = list(difflib.unified_diff(sa[k], sb[k], lineterm='', n=0))
            print(f'  (a) {k}: {len(sa[k])} / {len(sb[k])} lines, {sum(1 for x in d if x[0] in "+-" and not x.startswith(("+++","---")))} differing')
            if '-v' in sys.argv:
                for x in d[:40]: print('      ' + x)
        if ma.get(k) != mb.get(k):
            nm += 1
            print(f'  (b) {k}: {ma.get(k)} -> {mb.get(k)}')
    print(f'   (a) kernels whose instruction stream differs: {ns};  (b) kernels whose metadata differs: {nm};  stream lines compared: {sum(len(v) for v in sa.values())}')
    bad += ns + nm
print('TOTAL differences:', bad)
