#!/bin/bash
# The `library_ab` block of profiles/selected_split_time.json: A/Bs of two builds of the library in ONE session
# (processes alternate, as scripts/ab_lib.sh does), plus the launches per frame of the four legs.
#
#   bash scripts/selected_split_ab.sh ROUNDS_LIB PARENT_LIB [LINES.jsonl]      (from the repository root, on the GPU)
#   python scripts/selected_split_time.py --out profiles/selected_split_time.json     # the four-leg tables first,
#   python scripts/selected_split_time.py --merge-ab LINES.jsonl --out profiles/selected_split_time.json
#
# ROUNDS_LIB  liblidf_hip.so of this tree built with the development macro that sends the selected list through
#             the rank-1 ray rounds (in a copy of the tree, so that the tree's own library stays the shipped form):
#                 LIDF_EXTRA_HIPCC_FLAGS=-DLIDF_H_LIST_ROUNDS python implicit_depth_amd/csrc/build.py --force
# PARENT_LIB  liblidf_hip.so built from the parent commit's sources (`git archive <parent> | tar -x -C DIR`, then
#             `python implicit_depth_amd/csrc/build.py` in DIR)
# Keep both outside the tree's csrc/ (the ignored _b_*/ folders serve); LIDF_HIP_LIB selects the build per process.
#
#   list-tree / list-rounds          lidf_query f16x3 / selected on the one-candidate-per-ray scene (P = R = 76,800)
#                                    under rocprofv3 --kernel-trace: the call by device events, and the durations
#                                    of its two lidf_points_h_kernel launches (prob_dec, then offset_dec on the list)
#   headline-tree / headline-parent  f16x3 / all at 240 x 320 x 64: the existing launch against the parent commit
#   frame-<leg>                      kernel launches per eager one-stream frame, from a kernel trace of 4 frames
set -o pipefail
ROUNDS=${1:?the rounds build of liblidf_hip.so}
PARENT=${2:?the parent commit\'s liblidf_hip.so}
AB=${3:-selected_split_ab.jsonl}
S=scripts/selected_split_time.py
T=$(mktemp -d)
: > "$AB"
step() {  # step SECONDS command...: a time limit per GPU step; the script ends at the first step that fails
  timeout -k 10 "$@" || { echo "step failed ($?): $*" >&2; exit 1; }
}
for v in tree rounds tree rounds; do
  if [ $v = tree ]; then unset LIDF_HIP_LIB; else export LIDF_HIP_LIB=$ROUNDS; fi
  D=$T/list_$v$RANDOM
  step 240 rocprofv3 --kernel-trace -d "$D" -o r -- python $S --leg f16x3/selected --shape list --window 0.5 --tag list-$v >> "$AB"
  step 60 python $S --trace-db "$(find "$D" -name '*_results.db' | head -1)" --tag list-$v >> "$AB"
done
for v in tree parent tree parent; do
  if [ $v = tree ]; then unset LIDF_HIP_LIB; else export LIDF_HIP_LIB=$PARENT; fi
  step 240 python $S --leg f16x3/all --shape headline --tag headline-$v >> "$AB"
done
unset LIDF_HIP_LIB
for leg in f32/all f32/selected f16x3/all f16x3/selected; do
  D=$T/frame_$RANDOM
  step 240 rocprofv3 --kernel-trace -d "$D" -o r -- python $S --frame-leg $leg > /dev/null
  step 60 python $S --frames-db "$(find "$D" -name '*_results.db' | head -1)" --tag "frame-$leg" >> "$AB"
done
rm -rf "$T"
grep -c '^{' "$AB"
