"""Static instruction budget of the headline sampler kernel's two Toeplitz-table GEMM phases (no GPU needed: hipcc cross-compiles).

`nuts_kernel<11,2,1,false>` is compiled to assembly the way tools/isa_kernel.sh does it and cut into the phases of a round by
tools/isa_phase_mix.py.  An fp64 MFMA and a VALU instruction share the SIMD's issue slots, so every VALU instruction of the phases
[B1, B2) and [B3, B4) is serial time for both waves of the SIMD.  Before the lane table (bdrt_tile_s1.h::toep_lane_table_fill) the two
phases held 203 and 189 VALU instructions (MFMA not counted), nearly all of them address arithmetic that is the same in every round.
What a routine needs is one add per operand pointer where a block's pointers are set (about 15), four v_add_f64 and four address adds
per tile end, and a few instructions for the table reads -- well under 100 with what else lives in those phases (the activity flags,
the spectrum request, the epilogue's addresses) -- hence the bound: at most half of the former count, each.  The kernel must also keep
0 bytes of scratch and two waves per SIMD.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)
PARENT_VALU = {'forward GEMM': 203, 'backward GEMM': 189}


@pytest.mark.skipif(HIPCC is None, reason='hipcc not found')
def test_headline_gemm_phases_valu_budget(tmp_path):
    src = tmp_path / 'probe_11_2_1.hip'
    src.write_text('#include "bdrt_nuts16.h"\nnamespace bdrt { BDRT_NUTS16_DEFINE(11, 2, 1) }\n')
    asm = tmp_path / 'probe_11_2_1.s'
    subprocess.check_call([HIPCC, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-ffp-contract=fast',
                           '-mllvm', '-disable-machine-licm', '-mllvm', '-amdgpu-sched-strategy=max-ilp', '-w',
                           '-I' + os.path.join(ROOT, 'bayes_drt_amd', 'csrc'), '--offload-device-only', '-S', str(src), '-o', str(asm)])
    lines = asm.read_text().split('\n')
    # the production instantiation (PROF = false): its body, and the compiler's resource lines behind it
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
    valu, mfma = {}, {}
    for l in out.split('\n'):
        for name in PARENT_VALU:
            if l.startswith(name):
                toks = l[len(name):].split()          # VALU, then fp64 int_addr mov cmp_sel cross_lane sgpr_spill mfma ...
                valu[name], mfma[name] = int(toks[0]), int(toks[7])
    assert set(valu) == set(PARENT_VALU), out
    for name, parent in PARENT_VALU.items():
        print('%s: VALU %d (parent %d, bound %d), MFMA %d' % (name, valu[name], parent, parent // 2, mfma[name]))
        assert mfma[name] >= 40, (name, mfma[name])          # the GEMMs themselves are still in those phases
        assert valu[name] <= parent // 2, (name, valu[name])
