"""Static shape of what stands around the two Toeplitz-table GEMMs of the headline sampler kernel (no GPU needed: hipcc cross-compiles).

`nuts_kernel<11,2,1,false>` is compiled to assembly the way tests/test_isa_budget.py does it and cut into the phases of a round by
tools/isa_phase_mix.py.  An fp64 MFMA and a VALU instruction share the SIMD's issue slots, and what a wave executes behind its last MFMA
of [B1, B2) or [B3, B4) runs into the partner wave's MFMA stream or, in the wave that arrives last, with the whole workgroup waiting at
the barrier.  Before this file's change 72 / 36 VALU instructions stood there (the spectrum request's 64-bit address arithmetic, the
activity flags, the epilogue's operand addresses), all of them the same in every round, and the spectrum request was 12 flat loads:
a flat load counts on lgkmcnt, so the `s_waitcnt lgkmcnt(0)` in front of the barrier waited for their round trip to memory.

Checked here:
  * no flat load in [B1, B2) nor anywhere in the round loop;
  * VALU instructions (MFMA not counted) between a phase's last v_mfma and its barrier, in listing order: forward <= 24, backward <= 12
    (one third of 72 / 36: what has to be there is four v_add_f64 and four output addresses of the last piece, the lane-offset adds
    of the spectrum request and the flag compare);
  * the whole phases as isa_phase_mix.py reports them: forward <= 48 (half of 97), backward <= 32 VALU;
  * 0 bytes of scratch, two waves per SIMD.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)
TAIL_BOUND = {'forward GEMM': 24, 'backward GEMM': 12}          # parent: 72 / 36
PHASE_BOUND = {'forward GEMM': 48, 'backward GEMM': 32}         # parent: 97 / 52
VALU_CLASSES = ('fp64', 'int_addr', 'mov', 'cmp_sel', 'cross_lane', 'sgpr_spill')


def _instructions(lines):
    for l in lines:
        s = l.strip()
        if not s or s.startswith(';') or s.startswith('.') or s.endswith(':'):
            continue
        yield s


def compile_headline(tmp_path, extra=()):
    """-> (lines of the kernel body, resources) of nuts_kernel<11,2,1,false>"""
    src = tmp_path / 'probe_11_2_1.hip'
    src.write_text('#include "bdrt_nuts16.h"\nnamespace bdrt { BDRT_NUTS16_DEFINE(11, 2, 1) }\n')
    asm = tmp_path / 'probe_11_2_1.s'
    subprocess.check_call([HIPCC, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-ffp-contract=fast',
                           '-mllvm', '-disable-machine-licm', '-mllvm', '-amdgpu-sched-strategy=max-ilp', '-w',
                           '-I' + os.path.join(ROOT, 'bayes_drt_amd', 'csrc'), *extra, '--offload-device-only', '-S', str(src), '-o', str(asm)])
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
    return lines[start:end + 1], res


def cut_phases(body):
    """The round loop and its two GEMM phases as line ranges, cut exactly as tools/isa_phase_mix.py cuts them."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import isa_phase_mix as ipm
    finally:
        sys.path.pop(0)
    bars = [i for i, l in enumerate(body) if l.strip().startswith('s_barrier')]
    best = max(range(len(bars) - 4), key=lambda k: bars[k + 4] - bars[k + 3])
    b1, b2, b3, b4, end = bars[best], bars[best + 1], bars[best + 2], bars[best + 3], bars[best + 4]
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r'^(\.LBB\d+_\d+):', l.strip())] if m}
    span = (0, bars[best - 1], end)
    for i, l in enumerate(body):
        m = re.match(r'\s*s_c?branch\S*\s+(\.LBB\d+_\d+)', l)
        if m and m.group(1) in labels and labels[m.group(1)] < i and i - labels[m.group(1)] > span[0]:
            span = (i - labels[m.group(1)], labels[m.group(1)], i)
    return ipm.classify, {'round loop': (span[1], span[2]), 'forward GEMM': (b1, b2), 'backward GEMM': (b3, b4)}


def tail_valu(body, classify, lo, hi):
    """VALU instructions (MFMA not counted) behind the last v_mfma of body[lo:hi]; -> (count, the instructions, number of MFMAs)"""
    ins = list(_instructions(body[lo:hi]))
    mf = [i for i, s in enumerate(ins) if classify(s) == 'mfma']
    tail = [s for s in ins[mf[-1] + 1:] if classify(s) in VALU_CLASSES] if mf else []
    return len(tail), tail, len(mf)


@pytest.mark.skipif(HIPCC is None, reason='hipcc not found')
def test_headline_gemm_tails(tmp_path):
    body, res = compile_headline(tmp_path)
    print('resources:', res)
    assert res['ScratchSize'] == 0
    assert res['Occupancy'] == 2

    classify, cuts = cut_phases(body)
    # no flat load in the forward phase, nor anywhere else in the round loop
    for name in ('forward GEMM', 'round loop'):
        lo, hi = cuts[name]
        flat = [s for s in _instructions(body[lo:hi]) if s.split()[0].startswith('flat_load')]
        print('%s: %d flat loads' % (name, len(flat)))
        assert not flat, (name, flat)

    # VALU behind the phase's last MFMA, in front of its barrier
    for name, bound in TAIL_BOUND.items():
        lo, hi = cuts[name]
        n, tail, nmfma = tail_valu(body, classify, lo, hi)
        print('%s: %d VALU behind the last of %d MFMA (bound %d)' % (name, n, nmfma, bound))
        for s in tail:
            print('    ' + s)
        assert nmfma >= 40, (name, nmfma)
        assert n <= bound, (name, n)

    # the whole phases, as tools/isa_phase_mix.py reports them
    f = tmp_path / 'nuts_kernel_11_2_1.s'
    f.write_text('\n'.join(body))
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, 'tools', 'isa_phase_mix.py'), str(f), 'headline'], text=True)
    print(out)
    valu = {}
    for l in out.split('\n'):
        for name in PHASE_BOUND:
            if l.startswith(name):
                valu[name] = int(l[len(name):].split()[0])
    assert set(valu) == set(PHASE_BOUND), out
    for name, bound in PHASE_BOUND.items():
        print('%s: VALU %d (bound %d)' % (name, valu[name], bound))
        assert valu[name] <= bound, (name, valu[name])
