"""The phase stamps (ar-vae_amd/csrc/stamps.h) are compiled into no library that the suite loads, so nothing else watches them:
every family of tools/stamp.py has to type-check with its flag, and the tool's list of families has to be the one in csrc."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ar-vae_amd', 'csrc')

_spec = importlib.util.spec_from_file_location('stamp_tool', os.path.join(ROOT, 'tools', 'stamp.py'))
stamp_tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(stamp_tool)                     # needs neither torch nor a GPU
FAMILIES = stamp_tool.FAMILIES


def _csrc_text():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith(('.hip', '.h'))}


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_stamped_source_type_checks(family):
    """host and device passes of the family's source with its flag: exit status 0 and no warning (no code is generated).
    -Wno-unused-command-line-argument: hipcc itself passes --hip-link, which a run that links nothing reports as unused."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    f = FAMILIES[family]
    cmd = [hipcc, '--offload-arch=gfx950', '-std=c++17', '-Wall', '-Wno-unused-function', '-fsyntax-only', '-Wno-unused-command-line-argument',
           '-D' + f['flag'],
           os.path.join(CSRC, f['source'])]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    assert 'warning:' not in p.stdout, p.stdout


def test_the_tool_lists_the_flags_of_csrc():
    """an instrument without a tool entry, or a tool entry without an instrument, fails here"""
    in_csrc = set(re.findall(r'ARVAE_STAMPS_[A-Z0-9]+', ''.join(_csrc_text().values())))
    assert in_csrc == {f['flag'] for f in FAMILIES.values()}
    assert all(f['flag'] == 'ARVAE_STAMPS_' + name.upper() for name, f in FAMILIES.items())


def test_the_tool_reads_the_tables_as_declared():
    """the (rows, slots, words) the tool reads with are those of the family's ARVAE_STAMP_TABLE declaration, found in the
    family's source or a header it includes, under the family's flag"""
    text = _csrc_text()
    declared = {}
    for name, src in text.items():
        if name == 'stamps.h':
            continue
        for m in re.finditer(r'#ifdef (ARVAE_STAMPS_[A-Z0-9]+)\n(?:(?!#endif).*\n)*?.*\bARVAE_STAMP_TABLE(?:_ONLY)?\((\w+), (\d+), (\d+), (\d+)\)', src):
            assert m.group(2) not in declared, m.group(2)
            declared[m.group(2)] = (m.group(1), tuple(int(g) for g in m.group(3, 4, 5)), name)
    assert set(declared) == set(FAMILIES)
    for family, (flag, shape, where) in declared.items():
        f = FAMILIES[family]
        assert (flag, shape) == (f['flag'], tuple(f['shape'])), family
        assert where == f['source'] or f'#include "{where}"' in text[f['source']], family
        view = f.get('view', shape[:2])
        n = 1
        for d in view:
            n *= d
        assert n == shape[0] * shape[1] * shape[2], family
