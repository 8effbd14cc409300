#!/usr/bin/env python3
"""Did a host-side change leave the device code alone?  Per kernel symbol of the gfx950 code objects embedded in two builds of the
same objects (or libraries): scratch bytes, VGPRs, SGPRs, LDS bytes (the code object's notes, as scripts/kernel_resources.py reads
them) and the symbol's code size (its symbol table).  Needs no GPU.
    python scripts/kernel_code_compare.py PARENT_DIR NEW_DIR ah_groupby.o ah_hash_part.o > table.json
Exit status 1 when the sets of kernel symbols or any of the five values differ."""
import json, os, re, struct, subprocess, sys, tempfile

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def code_objects(path):
    data = open(path, "rb").read()
    pos = 0
    while True:
        pos = data.find(b"\x7fELF\x02\x01\x01", pos)
        if pos < 0:
            return
        hdr = data[pos:pos + 64]
        if struct.unpack_from("<H", hdr, 18)[0] != 224:  # EM_AMDGPU
            pos += 4
            continue
        e_shoff, = struct.unpack_from("<Q", hdr, 40)
        e_shentsize, e_shnum = struct.unpack_from("<HH", hdr, 58)
        size = e_shoff + e_shentsize * e_shnum
        yield data[pos:pos + size]
        pos += max(size, 1)


def kernels(path):
    out = {}
    for blob in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
            f.write(blob)
        notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True).stdout
        syms = subprocess.run([READELF, "--symbols", "--wide", f.name], capture_output=True, text=True).stdout
        os.unlink(f.name)
        sizes = {}
        for line in syms.splitlines():
            p = line.split()
            if len(p) >= 8 and p[3] == "FUNC":
                sizes[p[7]] = int(p[2], 0)
        for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, ""])[1]
            name = g("name")
            out[name] = {"scratch_bytes": int(g("private_segment_fixed_size")), "vgprs": int(g("vgpr_count")), "sgprs": int(g("sgpr_count")),
                         "lds_bytes": int(g("group_segment_fixed_size")), "code_bytes": sizes.get(name)}
    return out


def main():
    parent_dir, new_dir, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    table, same = {}, True
    for f in files:
        a, b = kernels(os.path.join(parent_dir, f)), kernels(os.path.join(new_dir, f))
        rows = []
        for name in sorted(set(a) | set(b)):
            pa, nb = a.get(name), b.get(name)
            rows.append({"kernel": name, "parent": pa, "new": nb, "same": pa == nb and pa is not None and pa["code_bytes"] is not None})
            same = same and rows[-1]["same"]
        table[f] = {"kernels": len(rows), "identical": all(r["same"] for r in rows), "rows": rows}
    json.dump({"identical": same, "objects": table}, sys.stdout, indent=1)
    print()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
