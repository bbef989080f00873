#!/usr/bin/env python3
"""isa_stream_cmp.py PARENT_DIR NEW_DIR [--files=a,b] [--rename=OLD:NEW,...] [-v]: per kernel of DIR/<file>.s (matched by name; --rename
replaces OLD by NEW in the parent's names first; files default to the window conv kernels) compare
(a) the stream of v_mfma / ds_ / global_ / buffer_ / scratch_ / s_barrier / s_waitcnt / s_sleep / s_cbranch / s_branch / s_endpgm lines with operands
(c) every line of the kernel's text (comments dropped, the kernel's own name and label indices neutralised)
(b) .vgpr_count .agpr_count .sgpr_count .vgpr_spill_count .sgpr_spill_count .private_segment_fixed_size .group_segment_fixed_size"""
import re, sys, difflib
PAT = re.compile(r'^\s*(v_mfma|ds_|global_|buffer_|scratch_|s_barrier|s_waitcnt|s_sleep|s_cbranch|s_branch|s_endpgm)')
META = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.vgpr_spill_count', '.sgpr_spill_count', '.private_segment_fixed_size', '.group_segment_fixed_size')
OPT = {a.split('=')[0]: a.split('=')[1] for a in sys.argv[3:] if '=' in a}
FILES = OPT.get('--files', 'conv_win,conv_win16,conv_win2').split(',')
RENAME = [r.split(':') for r in OPT.get('--rename', '').split(',') if r]
def parse(path, rename=()):
    streams, meta, cur = {}, {}, None
    text = open(path).read()
    for old, new in rename: text = text.replace(old, new)
    lines = text.split('\n')
    for ln in lines:
        m = re.match(r'^(_Z\w+):', ln)
        if m: cur = m.group(1); streams[cur] = []; full[path, cur] = []; continue
        if ln.startswith('.Lfunc_end'): cur = None; continue
        if cur and re.sub(r'\s*;.*$', '', ln).strip(): full[path, cur].append(re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r'\s*;.*$', '', ln.strip())))
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
full = {}
for f in FILES:
    pa, pb = f'{sys.argv[1]}/{f}.s', f'{sys.argv[2]}/{f}.s'
    sa, ma = parse(pa, RENAME); sb, mb = parse(pb)
    print(f'== {f}.hip: kernels {len(sa)} / {len(sb)}, metadata records {len(ma)} / {len(mb)}, names equal: {sorted(sa) == sorted(sb) and sorted(ma) == sorted(mb) and sorted(sa) == sorted(ma)}')
    if sorted(sa) != sorted(sb): bad += 1; print(f'  only in parent: {sorted(set(sa) - set(sb))}\n  only in new: {sorted(set(sb) - set(sa))}')
    ns = nm = nf = 0
    for k in sorted(sa):
        if k not in sb: continue
        if sa[k] != sb[k]:
            ns += 1
            d = list(difflib.unified_diff(sa[k], sb[k], lineterm='', n=0))
            print(f'  (a) {k}: {len(sa[k])} / {len(sb[k])} lines, {sum(1 for x in d if x[0] in "+-" and not x.startswith(("+++","---")))} differing')
            if '-v' in sys.argv:
                for x in d[:40]: print('      ' + x)
        if full[pa, k] != full[pb, k]: nf += 1; print(f'  (c) {k}: text differs')
        if ma.get(k) != mb.get(k):
            nm += 1
            print(f'  (b) {k}: {ma.get(k)} -> {mb.get(k)}')
    print(f'   (a) kernels whose instruction stream differs: {ns};  (b) kernels whose metadata differs: {nm};  (c) kernels whose full text differs: {nf};  stream lines compared: {sum(len(sa[k]) for k in sa if k in sb)}, text lines: {sum(len(full[pa, k]) for k in sa if k in sb)}')
    bad += ns + nm + nf
print('TOTAL differences:', bad)
