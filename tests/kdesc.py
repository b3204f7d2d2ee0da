"""Reading libzfp_hip.so without a GPU: ELF sections and symbols, and the
gfx950 code objects in its .hip_fatbin section (clang offload bundles of ELF
code objects) with their kernel descriptors (`<name>.kd`)."""
import struct

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _sections(elf):
    """(name, type, offset, size, link) of every section of an ELF64 image."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    hdrs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    stro = hdrs[shstrndx][4]
    out = []
    for h in hdrs:
        nm = elf[stro + h[0]: elf.index(b"\0", stro + h[0])].decode()
        out.append((nm, h[1], h[4], h[5], h[6]))
    return out


def _symbols(elf):
    secs = _sections(elf)
    names = set()
    for nm, typ, off, size, link in secs:
        if typ not in (2, 11):  # SHT_SYMTAB, SHT_DYNSYM
            continue
        stro = secs[link][2]
        for i in range(size // 24):
            st_name, = struct.unpack_from("<I", elf, off + i * 24)
            if st_name:
                names.add(elf[stro + st_name: elf.index(b"\0", stro + st_name)].decode())
    return names


def _device_kernels(lib_bytes):
    secs = {nm: (off, size) for nm, _, off, size, _ in _sections(lib_bytes)}
    off, size = secs[".hip_fatbin"]
    fb = lib_bytes[off: off + size]
    kernels, objects, i = set(), 0, 0
    while True:
        j = fb.find(MAGIC, i)
        if j < 0:
            break
        n, = struct.unpack_from("<Q", fb, j + 24)
        p = j + 32
        for _ in range(n):
            o, sz, tl = struct.unpack_from("<QQQ", fb, p)
            p += 24
            triple = fb[p: p + tl].decode()
            p += tl
            if "gfx950" in triple and sz:
                objects += 1
                kernels |= {s[:-3] for s in _symbols(fb[j + o: j + o + sz]) if s.endswith(".kd")}
        i = j + len(MAGIC)
    return kernels, objects


def _kernel_scratch(lib_bytes):
    """{kernel: private_segment_fixed_size} from the gfx950 kernel descriptors (.kd)."""
    secs = {nm: (off, size) for nm, _, off, size, _ in _sections(lib_bytes)}
    off, size = secs[".hip_fatbin"]
    fb = lib_bytes[off: off + size]
    out, i = {}, 0
    while True:
        j = fb.find(MAGIC, i)
        if j < 0:
            break
        n, = struct.unpack_from("<Q", fb, j + 24)
        p = j + 32
        for _ in range(n):
            o, sz, tl = struct.unpack_from("<QQQ", fb, p)
            p += 24
            triple = fb[p: p + tl].decode()
            p += tl
            if "gfx950" not in triple or not sz:
                continue
            elf = fb[j + o: j + o + sz]
            shoff, = struct.unpack_from("<Q", elf, 0x28)
            shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
            hdrs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + k * shentsize) for k in range(shnum)]
            for h in hdrs:
                if h[1] not in (2, 11):
                    continue
                stro = hdrs[h[6]][4]
                for k in range(h[5] // 24):
                    st_name, _, _, shndx, value, _ = struct.unpack_from("<IBBHQQ", elf, h[4] + k * 24)
                    nm = elf[stro + st_name: elf.index(b"\0", stro + st_name)].decode() if st_name else ""
                    if not nm.endswith(".kd") or shndx == 0 or shndx >= len(hdrs):
                        continue
                    sec = hdrs[shndx]
                    kd = sec[4] + (value - sec[3])  # file offset of the descriptor
                    out[nm[:-3]] = struct.unpack_from("<I", elf, kd + 4)[0]
        i = j + len(MAGIC)
    return out
