#!/bin/bash
# Register / scratch / occupancy listing of every k_admm_res2 instantiation (hipcc -Rpass-analysis=kernel-resource-usage):
#     tools/res2_resource_usage.sh [path/to/rqp_resident2.hip] > listing.txt
R=$(cd "$(dirname "$0")/.." && pwd)
SRC=${1:-$R/reluqp-py_amd/csrc/rqp_resident2.hip}
T=$(mktemp -d)
${HIPCC:-/opt/rocm/bin/hipcc} -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I$R/include -I$R/reluqp-py_amd/csrc -Rpass-analysis=kernel-resource-usage \
    -c "$SRC" -o $T/x.o 2>&1 | grep -E "Function Name|VGPRs:|AGPRs|ScratchSize|Occupancy" | sed -e 's/^.*remark: //' -e 's/^[^ ]*\.hip:[0-9:]* *//' -e 's/^ *//' -e 's/ \[-Rpass.*$//' |
    awk '/Function Name/ {name=$3; keep=(name ~ /k_admm_res2/); if (keep) { cmd="c++filt " name; cmd | getline d; close(cmd); sub(/\(SolveArgs.*/, "", d); printf "%s", d } next} keep {printf " | %s", $0} /Occupancy/ && keep {printf "\n"}'
rm -rf $T
