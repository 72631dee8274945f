# same-call A/B of tools/exp_ws64_layers.py between library builds: ab_ws64_libs.sh <clips> <lib> <lib> ...   (alternating, ROUNDS rounds -- default 2 --
# of READINGS readings of REPS launches; every run under its own time limit, the chain stops at the first one that fails)
CLIPS=${1:-128}; shift
LIBS=${@:-"musicfpaugment_amd/libmfpa_base.so musicfpaugment_amd/libmfpa.so"}
for i in $(seq ${ROUNDS:-2}); do for l in $LIBS; do
  echo "== $l"
  timeout -k 10 240 python tools/exp_ws64_layers.py --lib "$l" --clips "$CLIPS" --reps ${REPS:-5} --readings ${READINGS:-2} 2>&1 | grep -v amdgpu; rc=${PIPESTATUS[0]}
  [ "$rc" -eq 0 ] || exit "$rc"
done; done
