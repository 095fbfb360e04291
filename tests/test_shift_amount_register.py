"""No kernel of the built libgu.so shifts 64 bits by an amount that sits in the LAST register of its VGPR allocation.

On gfx950 such a shift (v_lshrrev_b64, v_lshlrev_b64, v_ashrrev_i64 with the amount in v63 of 64 registers, v31 of 32, ...) now and then
takes the low six bits of the register BEHIND the wave's allocation as its amount when other waves share the SIMD (docs/HISTORY.md
"64-bit shift by the last VGPR": the general rollout kernel's statistics-only stream launch moved envs by lut >> lane).  Where the
amount lands is the register allocator's choice and changes with any edit or compiler, so the library is read back after every build:
its gfx950 code objects are disassembled, and every 64-bit shift's amount register is compared with the kernel's VGPR count from the
code object's metadata.  No device; a few seconds."""
import glob
import os
import re
import subprocess

from griduniverse_amd import _lib

LLVM = os.path.join(os.path.dirname(os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')), '..', 'llvm', 'bin')
GRANULE = 8  # VGPRs are allocated in blocks of eight per lane (wave64, gfx90a and later)
SHIFT = re.compile(r'^\s+(v_lshrrev_b64|v_lshlrev_b64|v_ashrrev_i64) v\[\d+:\d+\], v(\d+),')
SYMBOL = re.compile(r'^[0-9a-f]+ <(\w+)>:')


def kernel_vgpr_counts(notes):
    """kernel -> .vgpr_count of a code object's metadata (llvm-readelf --notes: a kernel's fields follow its arguments', in alphabetical order)."""
    counts, name = {}, None
    for line in notes.splitlines():
        if line.startswith('    .name:'):
            name = line.split()[-1]
        elif line.startswith('    .vgpr_count:'):
            counts[name] = int(line.split()[-1])
    return counts


def last_register_shifts(disassembly, vgpr_count):
    """([(kernel, instruction)], shifts seen): the 64-bit shifts whose amount register is the last of the kernel's allocation."""
    found, seen, kernel = [], 0, None
    for line in disassembly.splitlines():
        if not line.startswith('\t'):
            m = SYMBOL.match(line)
            kernel = m.group(1) if m else kernel
        elif '64 ' in line[:16]:
            m = SHIFT.match(line)
            if m and kernel in vgpr_count:
                seen += 1
                allocated = -(-vgpr_count[kernel] // GRANULE) * GRANULE
                if int(m.group(2)) == allocated - 1:
                    found.append((kernel, line.split('//')[0].strip()))
    return found, seen


def test_the_scan_sees_the_shift_that_lost_envs():
    """The instruction as it stood in the failing kernel (64 registers, the amount in v63), one register off, and a kernel of 58."""
    text = ('0000000000001000 <k64>:\n\tv_lshrrev_b64 v[24:25], v63, s[8:9]    // 0\n\tv_lshrrev_b64 v[24:25], v62, s[8:9]\n'
            '0000000000002000 <k58>:\n\tv_lshrrev_b64 v[2:3], v57, s[8:9]\n\tv_lshlrev_b64 v[2:3], v63, v[4:5]\n\tv_lshrrev_b64 v[0:1], 3, v[2:3]\n')
    assert last_register_shifts(text, dict(k64=64, k58=58)) == ([('k64', 'v_lshrrev_b64 v[24:25], v63, s[8:9]'), ('k58', 'v_lshlrev_b64 v[2:3], v63, v[4:5]')], 4)


def test_no_kernel_shifts_64_bits_by_its_last_register(tmp_path):
    objdump, readelf = os.path.join(LLVM, 'llvm-objdump'), os.path.join(LLVM, 'llvm-readelf')
    assert os.path.exists(objdump) and os.path.exists(readelf), 'llvm-objdump / llvm-readelf are expected beside the hipcc that built the library: ' + LLVM
    lib = str(tmp_path / 'libgu.so')
    os.symlink(_lib.LIB_PATH, lib)
    subprocess.check_call([objdump, '--offloading', lib], cwd=str(tmp_path), stdout=subprocess.DEVNULL)  # (the code objects land beside the input)
    objects = sorted(glob.glob(lib + '.*gfx950*'))
    assert len(objects) >= 30, objects
    kernels, shifts, found = 0, 0, []
    for co in objects:
        notes = subprocess.run([readelf, '--notes', co], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
        vgpr_count = kernel_vgpr_counts(notes)
        text = subprocess.run([objdump, '-d', co], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
        bad, seen = last_register_shifts(text, vgpr_count)
        kernels, shifts, found = kernels + len(vgpr_count), shifts + seen, found + bad
    assert kernels > 500 and shifts > 5000, (kernels, shifts)  # (the scan read what it was meant to read)
    assert not found, '%d 64-bit shifts by the last allocated VGPR; the first: %s' % (len(found), found[:5])
