"""Static check of the power-scaling kernels (no GPU needed: hipcc cross-compiles): bdrt_powerscale.hip is compiled for gfx950
with the Makefile's flags for the post-sampling statistics, and every kernel of it must keep 0 bytes of scratch -- the sorted
positions a thread holds in registers (ps_cjs_kernel) and the eight running sums must not spill.  Only the compiler's resource
lines are read, as tests/test_isa_budget.py reads them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bayes_drt_amd', 'csrc')
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)
KERNELS = ('ps_sums_kernel', 'ps_weights_kernel', 'ps_cjs_kernel')


def _makefile_flags():
    """CXXFLAGS of the Makefile and what its rule for the post-sampling statistics adds; the rule must name the new object."""
    txt = open(os.path.join(CSRC, 'Makefile')).read()
    flags = re.search(r'^CXXFLAGS \?= (.*)$', txt, flags=re.M).group(1).replace('$(ARCH)', 'gfx950').split()
    rule = re.search(r'^([^\n]*bdrt_rank\.o[^\n]*): %\.o: %\.hip \$\(HDRS\)\n\t\$\(HIPCC\) \$\(CXXFLAGS\) (.*) -c \$< -o \$@$', txt, flags=re.M)
    assert rule and 'bdrt_powerscale.o' in rule.group(1).split()
    assert 'bdrt_powerscale.hip' in re.search(r'^SRCS := (.*)$', txt, flags=re.M).group(1).split()
    return flags + rule.group(2).split()


@pytest.mark.skipif(HIPCC is None, reason='hipcc not found')
def test_powerscale_kernels_keep_no_scratch(tmp_path):
    flags = _makefile_flags()
    assert '-ffp-contract=off' in flags
    asm = tmp_path / 'bdrt_powerscale.s'
    subprocess.check_call([HIPCC] + flags + ['-w', '--offload-device-only', '-S', os.path.join(CSRC, 'bdrt_powerscale.hip'), '-o', str(asm)])
    lines = asm.read_text().split('\n')
    seen = {}
    for name in KERNELS:
        start = next(i for i, l in enumerate(lines) if re.match(r'^_ZN4bdrt\d+%s.*:' % name, l))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
        for l in lines[end:]:
            m = re.match(r'^; ScratchSize: (\d+)', l)
            if m:
                seen[name] = int(m.group(1))
                break
    print('ScratchSize:', seen)
    assert set(seen) == set(KERNELS)
    assert all(v == 0 for v in seen.values()), seen
