"""CPU: every csrc/*.hpp includes what it uses, so a new translation unit can start with any of them.

For each header, the one-line unit `#include "<header>"` must pass the device-side syntax check with the product flags."""
import glob
import os
import shutil
import subprocess

import pytest

from multiagent_rl_amd import build_native

CSRC = os.path.join(build_native.HERE, 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason='hipcc not installed')


@pytest.mark.parametrize('header', sorted(os.path.basename(h) for h in glob.glob(os.path.join(CSRC, '*.hpp'))))
def test_header_compiles_alone(header, tmp_path):
    unit = tmp_path / 'unit.hip'
    unit.write_text('#include "%s"\n' % header)
    r = subprocess.run([HIPCC] + build_native.FLAGS + ['-I', CSRC, '-fsyntax-only', '--cuda-device-only', str(unit)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
