#!/usr/bin/env python3
"""Static instruction counts of the streamed LDS walk kernels, split by what the instructions are for.
usage: tools/walk_overhead_count.py rpt_traverse.s     (hipcc <HIPFLAGS of the Makefile> --cuda-device-only -S rust-path-tracer_amd/csrc/rpt_traverse.hip)

The compiler's loop comments ("in Loop: Header=BBk_n Depth=d") say which loop a basic block belongs to.  In a streamed LDS kernel
    the refill loop      is the outermost loop that holds a walk loop,
    a walk loop          is a loop one of whose own blocks loads plane records (ds_read_b128),
    a triangle loop      is a loop inside a walk loop,
and the blocks of a walk loop are told apart in text order by what they hold:
    loop head            the blocks ahead of the header label (trip counter, budget) and from the header to the first body: kind
                         classification, vote
    inner body           from the block with the plane loads up to the block that decides between descend and pop
    push / pop           the blocks behind it that read or write the stack (ds_read_u16, ds_write_b16) or the descriptor word, and the pop behind a leaf
    leaf set-up          from the block that decodes (count, first) (v_bfe_u32) to the triangle loop
    triangle iteration   the triangle loop
    refill path          every block of the refill loop outside its walk loops
A kernel has one walk loop per instantiation of lds_walk_run it inlines: the exact-division walk of the streamed lanes ("fast") and the walk a ray outside
the division guard is walked with alone ("ieee": v_div_scale in its inner body).  Counts are STATIC: instructions in the text, not instructions issued.
VALU = v_*; SALU = s_* without s_waitcnt / s_nop / s_sleep / s_barrier / s_endpgm and without scalar memory; LDS = ds_*; VMEM = global_* / buffer_* / flat_*.
The flattened walk of the streamed lanes (k_walk.h lds_stream_walk_run) stands in another text order — latch (the ballots and the loop's one exit, ahead of the header label:
loop head), vote, leaf set-up, triangle loop, inner body, push, and ONE pop site behind both bodies — and the same rules sort it: what follows the triangle loop up to the
plane loads (the end of the leaf body, the vote's second half) and what follows the stack store (the merged pop) is push / pop.
A leaf body WITHOUT a triangle loop (one triangle per leaf trip, lds_stream_walk_run RPT_LEAF_ONE) is `triangle iteration` too: from the block of the walk loop that
loads a triangle record (ds_read_b96) to the block that gives exec back what the leaf body's s_and_saveexec took; its set-up is part of it (`leaf set-up` 0).
`inner trip, total` = loop head + inner body + push / pop: what a trip of the inner step issues.  The last two columns are the region's cost at the unit costs of
tools/microbench/valu_rates.hip (profiles/r04_valu_pipes.txt, question 3): 3.7 per vector and 6.5 per scalar instruction; a change pays where their sum goes down."""
import re, subprocess, sys

REGIONS = ['loop head', 'inner body', 'push / pop', 'leaf set-up', 'triangle iteration', 'refill path']
TRIP = ['loop head', 'inner body', 'push / pop']
VALU_UNITS, SALU_UNITS = 3.7, 6.5
NOT_SALU = ('s_waitcnt', 's_nop', 's_sleep', 's_barrier', 's_endpgm', 's_load', 's_buffer_load')

def kind(ins):
    op = ins.split()[0]
    if op.startswith('v_'): return 'VALU'
    if op.startswith('ds_'): return 'LDS'
    if op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')): return 'VMEM'
    if op.startswith('s_') and not op.startswith(NOT_SALU): return 'SALU'
    return None

def kernels(text):
    """{symbol: [block]}; a block = dict(name, loop (header it is IN, or itself when it is a header), is_header, parents, ins)"""
    out, cur, blk = {}, None, None
    lines = text.split('\n')
    for i, raw in enumerate(lines):
        m = re.match(r'(_Z\w+):', raw)
        if m:
            cur = out.setdefault(m[1], [])
            blk = dict(name='entry', loop=None, is_header=False, parents=[], ins=[])
            cur.append(blk)
            continue
        if cur is None: continue
        m = re.match(r'(?:\.L(BB\d+_\d+):|; %bb\.(\d+):)\s*(;.*)?$', raw)
        if m:
            note, parents, j = m[3] or '', [], i + 1
            while j < len(lines) and re.match(r'\s+;', lines[j]):      # the header's comment goes on over the next lines
                note += ' ' + lines[j].strip()
                j += 1
            blk = dict(name=m[1] or 'bb.' + m[2], loop=None, is_header=False, parents=re.findall(r'Parent Loop (BB\d+_\d+)', note), ins=[])
            inl = re.search(r'in Loop: Header=(BB\d+_\d+)', note)
            if 'Loop Header' in note: blk['loop'], blk['is_header'] = blk['name'], True
            elif inl: blk['loop'] = inl[1]
            cur.append(blk)
            continue
        if raw.startswith('.Lfunc_end') or '.section' in raw:      # the kernel's text ends here
            cur = None
            continue
        ins = re.split(r';', raw)[0].strip()
        if ins and raw[:1].isspace() and not ins.startswith('.') and blk is not None: blk['ins'].append(ins)
    return {k: v for k, v in out.items() if any(b['ins'] for b in v)}

def count(blocks):
    c = dict(VALU=0, SALU=0, LDS=0, VMEM=0)
    for b in blocks:
        for ins in b['ins']:
            k = kind(ins)
            if k: c[k] += 1
    return c

def analyse(blocks):
    parent = {b['name']: (b['parents'][-1] if b['parents'] else None) for b in blocks if b['is_header']}
    def inside(loop, anc):
        while loop is not None:
            if loop == anc: return True
            loop = parent.get(loop)
        return False
    has = lambda b, pat: any(re.match(pat, i) for i in b['ins'])
    walks = sorted({b['loop'] for b in blocks if b['loop'] and has(b, r'ds_read_b128')}, key=lambda n: [x['name'] for x in blocks].index(n))
    walks = [w for w in walks if not any(inside(parent.get(w), v) for v in walks)]
    result = []
    for w in walks:
        regs = {r: [] for r in REGIONS[:5]}
        state, seen_header, leaf_exec, prev = 'loop head', False, None, None
        for b in blocks:
            if not inside(b['loop'], w): continue
            if b['loop'] != w:
                regs['triangle iteration'].append(b)
                state = 'push / pop'                      # behind the triangle loop: the leaf's pop
                continue
            own_prev, prev = prev, b
            if b['is_header']: seen_header, state = True, 'loop head'
            elif not seen_header: state = 'loop head'     # latch blocks stand ahead of the header label
            elif has(b, r'ds_read_b96'):                  # a leaf body WITHOUT a triangle loop (one triangle per leaf trip): its triangle test
                state = 'triangle iteration'
                saved = [re.match(r's_and_saveexec_b64 (s\[\d+:\d+\])', i) for i in (own_prev['ins'] if own_prev else [])]
                leaf_exec = ([m[1] for m in saved if m] or [None])[-1]
            elif state == 'triangle iteration' and leaf_exec and b['ins'][:1] == ['s_or_b64 exec, exec, ' + leaf_exec]:
                state = 'push / pop'                      # the lanes that sat the leaf trip out are back: the vote's second half
            elif has(b, r'ds_read_b128'): state = 'inner body'
            elif has(b, r'v_bfe_u32') : state = 'leaf set-up'
            elif state == 'inner body' and (has(b, r'ds_read_u16|ds_write_b16|ds_read_b32') or has(b, r'v_mov_b32_e32 v\d+, 0x4000')): state = 'push / pop'
            regs[state].append(b)
        ieee = any(has(b, r'v_div_scale') for b in regs['inner body'])
        result.append((w, 'ieee' if ieee else 'fast', {r: count(bs) for r, bs in regs.items()}))
    outer = {w: w for w in walks}
    for w in walks:
        while parent.get(outer[w]) is not None: outer[w] = parent[outer[w]]
    mains = set(outer.values())
    refill = [b for b in blocks if any(inside(b['loop'], m) for m in mains) and not any(inside(b['loop'], w) for w in walks)]
    return result, count(refill)

def main(path):
    ks = kernels(open(path).read())
    names = [k for k in ks if re.match(r'_Z\d+k_traverse_(nearest|shadow)_stream', k)]
    pretty = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    fmt = '    %-22s %6s %6s %5s %5s %9s %9s'
    units = lambda c: ('%.1f' % (VALU_UNITS * c['VALU']), '%.1f' % (SALU_UNITS * c['SALU']))
    for n, p in sorted(zip(names, pretty), key=lambda t: t[1]):
        walks, refill = analyse(ks[n])
        print(re.sub(r'\(.*', '', p).replace('void ', ''))
        for w, form, regs in walks:
            print('  walk loop %s (%s)' % (w, form))
            print(fmt % ('', 'VALU', 'SALU', 'LDS', 'VMEM', 'VALU x3.7', 'SALU x6.5'))
            for r in REGIONS[:5]: print(fmt % (r, regs[r]['VALU'], regs[r]['SALU'], regs[r]['LDS'], regs[r]['VMEM'], *units(regs[r])))
            trip = {k: sum(regs[r][k] for r in TRIP) for k in ('VALU', 'SALU', 'LDS', 'VMEM')}
            print(fmt % ('inner trip, total', trip['VALU'], trip['SALU'], trip['LDS'], trip['VMEM'], *units(trip)))
        print('  refill loop')
        print(fmt % ('refill path', refill['VALU'], refill['SALU'], refill['LDS'], refill['VMEM'], *units(refill)))
        whole = count(ks[n])
        print(fmt % ('whole kernel', *[whole[k] for k in ('VALU', 'SALU', 'LDS', 'VMEM')], *units(whole)))
        print()

if __name__ == '__main__':
    if len(sys.argv) != 2: sys.exit(__doc__)
    main(sys.argv[1])
