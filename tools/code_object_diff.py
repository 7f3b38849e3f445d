"""Kernel by kernel, are the gfx950 code objects embedded in two builds of libksfd_hip.so the same?

    python tools/code_object_diff.py <parent libksfd_hip.so> <new libksfd_hip.so>

Unbundles the gfx950 code object of each library (llvm-objcopy, clang-offload-bundler), hashes the bytes of every FUNC symbol in .text and
lists the kernels added, removed and changed.  For a changed kernel the disassemblies are compared line by line with addresses stripped:
a kernel whose only differences are literals of s_add_u32 / s_addc_u32 (pc-relative displacements to a table that moved) is reported as
'moved literals only'.  Works in a temporary directory; writes nothing next to the libraries."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/llvm/bin')


def code_object(so, tag, tmp):
    fat, co = os.path.join(tmp, tag + '.fatbin'), os.path.join(tmp, tag + '.co')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '-O', 'binary', '--only-section=.hip_fatbin', so, fat])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950',
                           '--input=' + fat, '--output=' + co, '--unbundle'])
    return co


def kernels(co):
    out = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '-sW', '-S', co], text=True)
    m = re.search(r'\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)', out)
    addr, off = int(m.group(1), 16), int(m.group(2), 16)
    data = open(co, 'rb').read()
    res = {}
    for line in out.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == 'FUNC' and f[6] != 'UND':
            a, sz = int(f[1], 16), int(f[2])
            res[f[7]] = hashlib.sha256(data[a - addr + off:a - addr + off + sz]).hexdigest()
    return res


def disassembly(co, sym):
    txt = subprocess.check_output([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', '--disassemble-symbols=' + sym, co], text=True)
    keep = []
    for line in txt.splitlines():
        line = re.sub(r'//.*', '', line).strip()
        if line and not line.endswith(':') and 'file format' not in line and not line.startswith('Disassembly'):
            keep.append(re.sub(r'^[0-9a-f]+:\s*', '', line))
    return keep


def main():
    with tempfile.TemporaryDirectory() as tmp:
        ca, cb = code_object(sys.argv[1], 'parent', tmp), code_object(sys.argv[2], 'new', tmp)
        a, b = kernels(ca), kernels(cb)
        print('kernels: parent %d, new %d; identical bytes: %d' % (len(a), len(b), sum(1 for k in a if b.get(k) == a[k])))
        for k in sorted(k for k in a if k not in b):
            print('removed  %s' % k)
        for k in sorted(k for k in b if k not in a):
            print('added    %s' % k)
        for k in sorted(k for k in a if k in b and a[k] != b[k]):
            da, db = disassembly(ca, k), disassembly(cb, k)
            diff = [(x, y) for x, y in zip(da, db) if x != y]
            lit = len(da) == len(db) and all(re.sub(r'0x[0-9a-f]+', '', x) == re.sub(r'0x[0-9a-f]+', '', y) and x.startswith(('s_add_u32', 's_addc_u32')) for x, y in diff)
            print('changed  %s: %d of %d lines differ%s' % (k, len(diff) + abs(len(da) - len(db)), len(da), ' -- moved literals only' if lit else ''))
            for x, y in diff[:4]:
                print('           %s  ->  %s' % (x, y))


if __name__ == '__main__':
    main()
