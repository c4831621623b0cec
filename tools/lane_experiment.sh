#!/bin/bash
# Quick-turnaround tuning build of the lane-per-problem kernel (qp_lane.hip) into restartsqp_amd/lib/librsqp_exp.so;
# select it with RSQP_LIB=<path>. Extra compiler flags as arguments (e.g. -DRSQP_STAMPS, -DRSQP_LANE_XVOTE=<bits>,
# -DRSQP_LANE_WT=<bits>, -DRSQP_LANE_NOSTORE=<bits>: a timing-only build that leaves its pools unwritten).
set -e
cd "$(dirname "$0")/.."
OBJ=restartsqp_amd/lib/obj
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -x hip "$@" -c restartsqp_amd/csrc/qp_lane.hip -o $OBJ/qp_lane_exp.o
# (every other object of the product build, whatever translation units it has: run the product build first)
OTHERS=$(ls $OBJ/*.o | grep -v -e '/qp_lane\.o$' -e '/qp_lane_exp\.o$')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o restartsqp_amd/lib/librsqp_exp.so $OBJ/qp_lane_exp.o $OTHERS
echo built restartsqp_amd/lib/librsqp_exp.so
