"""The 16-bit build selection guards, without a GPU: a library of the other 16-bit flavour than DAT_H16 is refused at import (it
would read every 16-bit tensor in the wrong format), and the Trainer refuses the inference-only 16-bit modes."""
import os
import subprocess
import sys
import types

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_library_of_the_other_16_bit_format_is_refused_at_import():
    env = dict(os.environ, DAT_H16='fp16', DAT_LIB=os.path.join(REPO, 'detectandtrack_amd', 'libdat_hip.so'), PYTHONPATH=REPO)
    p = subprocess.run([sys.executable, '-c', 'import detectandtrack_amd.libdat'], env=env, cwd=REPO, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    err = p.stderr.decode()
    assert p.returncode != 0, 'the bf16 library was accepted under DAT_H16=fp16'
    assert 'AssertionError' in err and 'DAT_LIB=' in err and 'DAT_H16=fp16' in err and 'holds the bf16 build' in err, err[-2000:]
    # and the matching pair imports
    env['DAT_LIB'] = os.path.join(REPO, 'detectandtrack_amd', 'libdat_hip_f16.so')
    p = subprocess.run([sys.executable, '-c', 'import detectandtrack_amd.libdat as L; assert L.lib().dat_h16_format() == 1'], env=env,
                       cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]


@pytest.mark.parametrize('mode', ['fp16', 'bf16x3'])
def test_trainer_refuses_the_inference_only_modes(mode):
    from detectandtrack_amd.training import Trainer
    with pytest.raises(AssertionError, match=r"cfg.HIP.DTYPE '%s' is an inference mode \(train in 'bf16' or 'fp32'\)" % mode):
        Trainer(None, types.SimpleNamespace(dtype=mode))
