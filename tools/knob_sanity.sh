# Off-arms of the planner switches still give golden-green models (a knob that rots is worse than no knob).  Run on a GPU box:
#   tools/knob_sanity.sh [dccrn | fsn]      (default: both groups)
# The table returns to SEFD_TUNING's pairs after every test (tuning.clear()), so every selected test runs on the off-arm.  Stops at the first arm
# that is not green: nothing more is started on a GPU that may have faulted.
cd "$(dirname "$0")/.."
run() {
  echo "== $1"
  SEFD_TUNING=$1 timeout -k 10 900 python -m pytest tests/test_gpu_model.py -x -q -m gpu -k "$2" 2>&1 | tail -1
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ]; then echo "$1: exit status $rc, stopping"; exit $rc; fi
}
if [ "${1:-dccrn}" = dccrn ]; then
  for kn in "ENC0_BNFUSE=0" "ENC0_DIRECT=0" "ENC0_WG_SLOTS=1024"; do run $kn "golden and not fsn"; done
fi
if [ "${1:-fsn}" = fsn ]; then
  for kn in "FSN_WGCAT2=0" "ONES_MFMA=0" "FSN_HOLD=1"; do run $kn "fsn or FullSubNet or subband"; done
fi
