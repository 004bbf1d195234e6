#!/bin/bash
# Register and scratch use of the library's kernels, read from the gfx950 code object inside
# pylbl_amd/liblbl_amd.so (no GPU needed).  Usage: scripts/checks/kernel_registers.sh [pattern]
# (a substring of the mangled name: "path_" lists the sweeps -- path_sweep_kernel,
# path_radiance_kernel, path_flux_kernel, path_jacobian_kernel -- in both instantiations;
# "two_stream" the shortwave two-stream kernels, "thermal" the longwave ones: thermal_up_kernel and
# thermal_down_kernel, vector and scalar rows, each with the source of the level temperatures
# (Lb0E as the second template argument) and with the linear-in-tau one (Lb1E); the last template
# argument of the two-stream kernels is Lb1E with the spectral scatterer and Lb0E with the grey one;
# "thermal_radiance" thermal_view_kernel of lbl_path_thermal_radiance alone, vector and scalar rows;
# "solar_radiance" solar_view_kernel of lbl_path_solar_radiance likewise; each lists the grey
# instantiations (Lb0E as the second template argument) and the spectral ones of
# lbl_path_thermal_radiance_spectral and lbl_path_solar_radiance_spectral (Lb1E); "view_kernel" all
# eight: DESIGN.md section 30 has their table, and none may show scratch; "thermal_view" the four
# of thermal_view_kernel and the two of thermal_view_source_kernel, the view sweep of
# lbl_path_thermal_radiance_source: DESIGN.md section 31; "thermal_observer" the eight of
# thermal_observer_kernel, the sweep of lbl_path_thermal_radiance_observer -- vector or scalar
# rows, isothermal or linear-in-tau source, looking down or up as the three template arguments:
# DESIGN.md section 32 has their table, and none may show scratch).
# Also prints the md5 of the device code's .text: unchanged by edits that only move host code.
set -e
LIB=${LIB:-pylbl_amd/liblbl_amd.so}
TMP=$(mktemp -d)
LLVM=/opt/rocm/lib/llvm/bin
$LLVM/llvm-objcopy --dump-section .hip_fatbin=$TMP/fatbin $LIB
$LLVM/clang-offload-bundler --unbundle --type=o --input=$TMP/fatbin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$TMP/co
$LLVM/llvm-objcopy --dump-section .text=$TMP/text $TMP/co
echo "device .text md5: $(md5sum < $TMP/text | cut -d' ' -f1)"
$LLVM/llvm-readelf --notes $TMP/co | python3 -c "
import re, sys
text = sys.stdin.read()
pattern = sys.argv[1] if len(sys.argv) > 1 else ''
pattern = {'thermal_radiance': 'thermal_view_kernel',
           'solar_radiance': 'solar_view_kernel'}.get(pattern, pattern)
for block in text.split('- .agpr_count')[1:]:
    name = re.search(r'\.name:\s+(\S+)', block)
    if not name or pattern not in name.group(1):
        continue
    get = lambda key: (re.search(r'\.' + key + r':\s+(\d+)', block) or [None, '?'])[1]
    print('%-110s vgpr %3s sgpr %3s spill(v/s) %s/%s scratch %s lds %s' % (
        name.group(1)[:110], get('vgpr_count'), get('sgpr_count'), get('vgpr_spill_count'),
        get('sgpr_spill_count'), get('private_segment_fixed_size'), get('group_segment_fixed_size')))
" "$1"
rm -rf $TMP
