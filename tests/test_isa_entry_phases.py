"""Static instruction budget of the headline sampler kernel's two element-wise entry phases (no GPU needed: hipcc cross-compiles).

`nuts_kernel<11,2,1,false>` is compiled to assembly the way tests/test_isa_budget.py does it and cut into the phases of a round by
tools/isa_phase_mix.py.  In [loop head, B1) (parameters P1 + prior chain P2) and [B2, B3) (likelihood P3) both waves of a SIMD are in
element-wise code, so every VALU instruction there is time.  The arithmetic of the two phases is fixed (1131 and 349 fp64
instructions: the evaluator is held to the parent's bits); what this test bounds is what stands around it -- integer / address
instructions, compares / selects and moves.  Before the lane bases of P1 and P3 (bdrt_tile_s1.h: BDRT_P1_LANE_BASE,
BDRT_P1_STATIC_PRED, BDRT_P3_LANE_BASE) the two phases held 377 and 194 of them: a clamp `k < K ? k : 0` and an address of its own per
row and array, a compare and selects for every row.  With the rows of an array at immediate offsets from one lane base, and the
range tests of the rows below s1_kmin(NJ) gone, they hold 334 and 136 (profiles/r09/isa_phase_mix.txt).

The bounds: P3 at the count achieved plus a quarter (the slack of tests/test_isa_gemm_tails.py), 170, which is below the parent's 194
(a build with P3's rows clamped again holds 194).  For [loop head, B1) a quarter on top of 334 would lie above the parent's 377 and
bound nothing: there the bound is 350, about a third of the way from what was achieved to the parent.  A build with the parameter
reads clamped again holds 359 there, one with the range tests of every row 356: neither passes.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)
PHASES = {'P1 + P2 (parameters, prior chain)': dict(fp64=1131, parent=377, bound=350),
          'P3 (likelihood)': dict(fp64=349, parent=194, bound=170)}


@pytest.mark.skipif(HIPCC is None, reason='hipcc not found')
def test_headline_entry_phases_overhead_budget(tmp_path):
    src = tmp_path / 'probe_11_2_1.hip'
    src.write_text('#include "bdrt_nuts16.h"\nnamespace bdrt { BDRT_NUTS16_DEFINE(11, 2, 1) }\n')
    asm = tmp_path / 'probe_11_2_1.s'
    subprocess.check_call([HIPCC, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-ffp-contract=fast',
                           '-mllvm', '-disable-machine-licm', '-mllvm', '-amdgpu-sched-strategy=max-ilp', '-w',
                           '-I' + os.path.join(ROOT, 'bayes_drt_amd', 'csrc'), '--offload-device-only', '-S', str(src), '-o', str(asm)])
    lines = asm.read_text().split('\n')
    start = next(i for i, l in enumerate(lines) if re.match(r'^_ZN4bdrt11nuts_kernelILi11ELi2ELi1ELb0EE.*:', l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
    res = {}
    for l in lines[end:]:
        m = re.match(r'^; (ScratchSize|Occupancy|NumVgprs): (\d+)', l)
        if m and m.group(1) not in res:
            res[m.group(1)] = int(m.group(2))
        if len(res) == 3:
            break
    print('resources:', res)
    assert res['ScratchSize'] == 0
    assert res['Occupancy'] == 2

    body = tmp_path / 'nuts_kernel_11_2_1.s'
    body.write_text('\n'.join(lines[start:end + 1]))
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, 'tools', 'isa_phase_mix.py'), str(body), 'headline'], text=True)
    print(out)
    seen = {}
    for l in out.split('\n'):
        for name in PHASES:
            if l.startswith(name):
                toks = [int(t) for t in l[len(name):].split()]      # VALU, then fp64 int_addr mov cmp_sel cross_lane sgpr_spill mfma ...
                seen[name] = dict(fp64=toks[1], overhead=toks[2] + toks[3] + toks[4], mfma=toks[7])
    assert set(seen) == set(PHASES), out
    for name, want in PHASES.items():
        got = seen[name]
        print('%s: fp64 %d (parent %d), int_addr + mov + cmp_sel %d (parent %d, bound %d)'
              % (name, got['fp64'], want['fp64'], got['overhead'], want['parent'], want['bound']))
        assert got['mfma'] == 0, (name, got)                      # the cut is where it is meant to be: no GEMM in these phases
        assert got['fp64'] == want['fp64'], (name, got)           # the arithmetic is the parent's
        assert got['overhead'] <= want['bound'], (name, got)
