# A/B build of the conv kernels only: bash tools/build_voc_variant.sh NAME "-DFLAG=.. -DFLAG2=.."  ->  spark-tts_amd/sparkmi/ab/libsparkmi_NAME.so
# (smi_net.hip -- the one unit that holds the conv / LayerNorm kernels, SMI_CB_OCC among its switches -- recompiled with the flags;
# every other object of the diagnostics build reused as built by make)
set -e
cd "$(dirname "$0")/../spark-tts_amd/csrc"
name=$1; flags=$2
mkdir -p ab/$name ../sparkmi/ab
CXXFLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -I../../include -I. -Wall -Wno-unused-function -ffp-contract=off -mllvm -amdgpu-kernarg-preload-count=16 -DSMI_DIAG"
/opt/rocm/bin/hipcc $CXXFLAGS $flags -c smi_net.hip -o ab/$name/smi_net.o
others=$(ls diag/d_smi_*.o | grep -v '/d_smi_net\.o$')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../sparkmi/ab/libsparkmi_$name.so ab/$name/smi_net.o $others diag/diag_*.o
echo built ../sparkmi/ab/libsparkmi_$name.so
