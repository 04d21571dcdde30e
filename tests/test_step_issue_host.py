"""CPU test of the single handle's host decisions (chsimpy_amd/csrc/chs_step_host.h: how a call is entered, what is
constant over its steps, what one step of the fused pipeline issues) against an independent model of the launch logic
they replaced.  Nothing here touches a device."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_decisions_against_a_model_of_the_launch_logic(tmp_path):
    """tests/step_issue_model.cpp: step_issue and call_entry compared with the model over every combination of their
    inputs, then calls of 1, 2, 3 and 6 steps walked with the pending tail carried along -- every record and every
    time-step control runs exactly once, nothing is pending behind the last step, U is stored wherever something reads
    it.  Host C++ only, compiled with the build's compiler."""
    from chsimpy_amd import _build
    exe = str(tmp_path / 'step_issue_model')
    subprocess.run([os.environ.get('HIPCC', 'hipcc'), '-x', 'c++', '-std=c++17', '-O1', '-Wall', '-I' + _build.CSRC,
                    os.path.join(ROOT, 'tests', 'step_issue_model.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and ' 0 failures' in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[-4]) > 300000      # (the exhaustive comparison ran)
    # the header is host code: nothing of HIP in it, and the test program includes nothing else of the library
    hdr = open(os.path.join(_build.CSRC, 'chs_step_host.h')).read()
    assert re.findall(r'#include\s*([<"][^>"]+[>"])', hdr) == ['<stdint.h>']
    cpp = open(os.path.join(ROOT, 'tests', 'step_issue_model.cpp')).read()
    assert re.findall(r'#include\s*"([^"]+)"', cpp) == ['chs_step_host.h']
