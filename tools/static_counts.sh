#!/bin/bash
# Static instruction counts of the step kernel instantiations in the current sources (diagnostic; hipcc only, no GPU):
#   bash tools/static_counts.sh [extra hipcc flags]
TOOLS="$(cd "$(dirname "$0")" && pwd)"
cd "$TOOLS/../everglades-ai-wargame_amd/csrc"
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math "$@" -S --cuda-device-only -o /tmp/evg_static.s evg_kernels.hip 2>/dev/null
python3 - "$TOOLS" <<'P'
import sys
sys.path.insert(0, sys.argv[1])
import _prof
lines = open('/tmp/evg_static.s').read().split('\n')
for tag, name in (("persistent f32", _prof.step_kernel_symbol("persistent")), ("single-turn f32", _prof.step_kernel_symbol("single_turn"))):
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ':'))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith('.end_amdhsa_kernel') or lines[i].strip().startswith('.section'))
    c = dict(valu=0, salu=0, lds=0, vmem=0, waitcnt=0)
    for l in lines[start:end]:
        t = l.strip()
        if t.startswith('v_'): c['valu'] += 1
        elif t.startswith('s_waitcnt'): c['waitcnt'] += 1
        elif t.startswith('s_'): c['salu'] += 1
        elif t.startswith('ds_'): c['lds'] += 1
        elif t.startswith('global_') or t.startswith('buffer_') or t.startswith('flat_'): c['vmem'] += 1
    print(tag, c)
P
