"""Host compiles for the CPU tests: a plan header of red_gym_amd/csrc with a small extern "C" shim as a shared library loaded with
ctypes (build_shim), and a small C program against include/f110_hip.h whose output the ABI check reads (run_c)."""
import ctypes
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'red_gym_amd', 'csrc')
COMPILERS = {'c++': ('g++', 'c++', '/opt/rocm/llvm/bin/clang++'), 'c': ('gcc', 'cc', '/opt/rocm/llvm/bin/clang')}

# what the plan headers call on a refusal (the library's own is in f110_handle.hip): a shim that includes one prepends this
FAIL_SHIM = r'''
#include <cstdarg>
#include <cstdio>
#include <cstring>

static char g_msg[512];
int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char *shim_message() { return g_msg; }
'''


def compiler(lang='c++'):
    for path in filter(None, map(shutil.which, COMPILERS[lang])):
        return path
    raise RuntimeError('no host %s compiler (%s) found' % (lang.upper(), ', '.join(COMPILERS[lang])))


def _compile(tmp_dir, name, source, lang, flags):
    src, out = os.path.join(str(tmp_dir), name + '.' + lang.replace('+', 'p')), os.path.join(str(tmp_dir), name)
    with open(src, 'w') as f:
        f.write(source)
    subprocess.run([compiler(lang)] + flags + ['-o', out, src], check=True)
    return out


def build_shim(tmp_dir, name, source, lang='c++'):
    """Compiles `source` against csrc/ into a shared library in tmp_dir and loads it."""
    return ctypes.CDLL(_compile(tmp_dir, 'lib%s.so' % name, source, lang, ['-std=c++17' if lang == 'c++' else '-std=c99', '-O1', '-Wall', '-shared', '-fPIC', '-I', CSRC]))


def run_c(tmp_dir, name, source):
    """Compiles `source` as strict C99 against include/ into a program, runs it and returns what it printed."""
    exe = _compile(tmp_dir, name, source, 'c', ['-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include')])
    return subprocess.run([exe], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
