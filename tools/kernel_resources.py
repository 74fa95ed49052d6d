"""usage: python tools/kernel_resources.py file.hip [extra hipcc flags] -> per kernel: VGPRs, scratch bytes/lane, occupancy, spills
The attention objects are built with extra flags (csrc/Makefile, EXTRA): report on the shipped code object with
    python tools/kernel_resources.py svt_speechbrain_amd/csrc/attention_drop.hip -mllvm -amdgpu-mfma-vgpr-form -fno-honor-nans [-DSVT_OPERAND_F16]"""
import re, subprocess, sys
out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=fast", "-fPIC", "-std=c++17", "-c",
                      sys.argv[1], "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"] + sys.argv[2:], capture_output=True, text=True).stderr
name, d = None, {}
keys = {"VGPRs": "vgpr", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occ", "VGPRs Spill": "spill"}
for l in out.splitlines():
    m = re.search(r"Function Name: (\S+)", l)
    if m:
        name = m.group(1); d[name] = {}
    for k, short in keys.items():
        m = re.search(r"remark:\s+" + re.escape(k) + r": (\d+)", l)
        if m and name:
            d[name][short] = m.group(1)
for n, v in d.items():
    dn = subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip()
    dn = dn.replace("svt::(anonymous namespace)::", "").replace("void ", "")[:60]
    print(f"{dn:60s} vgpr {v.get('vgpr','?'):>4s} scratch {v.get('scratch','?'):>4s} occ {v.get('occ','?')} spill {v.get('spill','?')}")
