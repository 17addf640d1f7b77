// ntt_fwd_sealed.hip -- the forward direction of the sealed transforms (ntt_sealed_io.hpp): the kernels of
// fhe_ntt_forward_sealed, in a translation unit of their own so that the two directions compile side by side.
//
// Two-launch sizes (N >= 2^13): the forward column pass with the input digest, k_ntt_seal_finish (ntt_sealed.hip) for the input
// rows' verdicts, the forward row pass with the output digest.  Below 2^13 the single pass carries both.  Without an output seal
// the second launch is the checked transform's own kernel.
#include "ntt_sealed_io.hpp"

namespace fhe {

template hipError_t launch_ntt_sealed_dir<false>(hipStream_t, const PassArgs &, const SealIoArgs &, int, int, int, const NttSealIn &);

} // namespace fhe
