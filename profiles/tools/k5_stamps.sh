#!/bin/bash
# diagnostic: phase shares of the level-0 folded k_blur_solve launch from in-kernel stamps, and the drain timeline of the
# three level-0 launches without and with taper (a separate -DFFL_STAMP build).  Each GPU step has its own time limit and
# the next one only starts when it ended well; the normal library is rebuilt whatever happened.
cd "$GRAFT_REPO_ROOT"
(cd funscript_flow_amd/csrc && rm -f kernels_farneback.o && make EXTRA=-DFFL_STAMP > /dev/null 2>&1) || { echo build failed; exit 1; }
timeout -k 10 120 python profiles/tools/k5_stamps.py &&
timeout -k 10 120 python profiles/tools/k5_drain.py taper=0 &&
timeout -k 10 120 python profiles/tools/k5_drain.py taper=1
rc=$?
(cd funscript_flow_amd/csrc && rm -f kernels_farneback.o && make > /dev/null 2>&1)
exit $rc
