// Live kernel timing (profiling aid for bench.py's roofline object): while
// on, the launches of a few hot kernels are bracketed by timing events on the
// stream they are launched on; read() resolves the finished pairs into a
// total duration and a launch count.  Off by default (two event records per
// timed launch when on).  Implemented in msm_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tmv {
namespace ktimer {

enum Kernel : int {
  kAccum = 0, kWpart = 1, kPrep = 2, kSecpPrep = 3, kSecpVerify = 4,
  kMerkleLeavesLong = 5, kMerkleTreeLevels = 6, kMerkleAunts = 7, kMerkleVerify = 8, kMerkleLeaves = 9,
  kCommitLeaves = 10, kVoteExtSignbytes = 11, kSecpKeyTable = 12, kSecpPrepCached = 13, kSecpVerifyComb = 14,
  kMerkleDigestsLong = 15, kMerkleValueOps = 16, kResultLeaves = 17,
  kSpanLeaves = 18, kValsetSpanLeaves = 19,
  kCount = 20
};

void set(bool on);
bool on();
// begin() returns a token (nullptr when off); end() records the closing event.
void *begin(Kernel k, hipStream_t s);
void end(void *token, hipStream_t s);
// Waits for the recorded pairs of kernel k, adds them to *ms / *launches and
// forgets them.  0 or a HIP error.
int read(Kernel k, double *ms, uint64_t *launches);

}  // namespace ktimer
}  // namespace tmv
