"""Compare the gfx950 kernel bodies of two builds of libmaskdit_hip.so instruction by instruction.

    python tools/isa_diff.py OLD.so NEW.so [--filter gemm_nt8_kernel]

Extracts the device code objects (llvm-objdump --offloading), disassembles them and reports the kernels that are new,
gone, or whose instruction streams differ.  The displacement of an `s_getpc_b64` + `s_add_u32` pair (the PC-relative
address of a global, which moves whenever any other code in the object grows) is normalised away, as is trailing
`s_nop` padding.  Used to show that adding instantiations to a kernel template leaves the existing ones unchanged."""
import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = '/opt/rocm/llvm/bin/llvm-objdump'


def demangle(name):
    try:
        return subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip() or name
    except OSError:
        return name


def kernels(lib):
    tmp = tempfile.mkdtemp()
    try:
        dst = os.path.join(tmp, 'lib.so')
        shutil.copy(lib, dst)
        subprocess.run([OBJDUMP, '--offloading', dst], cwd=tmp, capture_output=True, check=True)
        out = {}
        for f in sorted(glob.glob(dst + '.*amdgcn*gfx950')):
            txt = subprocess.run([OBJDUMP, '-d', '--no-show-raw-insn', '--no-leading-addr', f], capture_output=True,
                                 text=True, check=True).stdout
            cur, prev = None, ''
            for line in txt.splitlines():
                m = re.match(r'^(?:[0-9a-f]+ )?<(\S+)>:', line)
                if m:
                    cur = m.group(1)
                    out[cur] = []
                    continue
                ins = re.sub(r'//.*', '', line).strip()
                if not cur or not ins or ins == '...':
                    continue
                if prev.startswith('s_getpc_b64') and ins.startswith('s_add_u32'):
                    ins = re.sub(r'0x[0-9a-f]+$', '<pcrel>', ins)
                out[cur].append(ins)
                prev = ins
        for k, v in out.items():
            while v and v[-1] == 's_nop 0':
                v.pop()
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--filter', default='', help='substring of the demangled kernel name')
    a = ap.parse_args(argv)
    old, new = kernels(a.old), kernels(a.new)
    sel = lambda d: {k: v for k, v in d.items() if a.filter in demangle(k)}
    old, new = sel(old), sel(new)
    common = sorted(set(old) & set(new))
    changed = [k for k in common if old[k] != new[k]]
    for k in sorted(set(new) - set(old)):
        print(f'new      {demangle(k)} ({len(new[k])} instructions)')
    for k in sorted(set(old) - set(new)):
        print(f'gone     {demangle(k)}')
    for k in common:
        print(f'{"CHANGED" if k in changed else "same":8s} {demangle(k)} ({len(old[k])} -> {len(new[k])} instructions)')
    print(f'{len(common)} kernels in both builds, {len(changed)} changed')
    return 1 if changed else 0


if __name__ == '__main__':
    sys.exit(main())
