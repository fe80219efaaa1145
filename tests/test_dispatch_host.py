"""ar-vae_amd/csrc/dispatch.h (with_bool / with_int: a run-time value picks a kernel instantiation) is host-only code: the
stand-alone program next to this file includes nothing else of the library, is built with the host compiler under the address and
undefined-behaviour sanitizers, and runs as a child process.  No GPU, no hipcc."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'ar-vae_amd', 'csrc')


def _host_compiler():
    for name in (os.environ.get('CXX'), 'c++', 'g++', 'clang++'):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_dispatchers_call_the_matching_constant_once_and_report_an_unlisted_value(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'dispatch_host')
    version = subprocess.run([cxx, '--version'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    # the sanitizer runtimes linked into the program (clang's default): it starts the same whatever the environment preloads
    static_rt = [] if 'clang' in version else ['-static-libasan', '-static-libubsan']
    cmd = [cxx, '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g'] + static_rt + \
          ['-I', CSRC, os.path.join(HERE, 'dispatch_host_main.cpp'), '-o', exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert ran.returncode == 0, ran.stdout
    assert 'dispatch.h: ok' in ran.stdout, ran.stdout
