// capi.hip -- the C ABI of libbee2hip.so (declared in include/bee2hip.h).
//
// Host side of the engine: argument checks and state bookkeeping mirror bee2's
// C functions line for line in *behaviour* (same names, same state layouts, same
// error codes).  Every batch / _dev / _multi entry point and every bign operation evaluates its primitives in
// kernels; the bee2 drop-in symbols do so too, except for small single calls, which take the host path of
// host_small.hpp ("host path for small single calls" below says exactly when).
// Split by primitive in round 5 (one translation unit still: the files below are included in this order, nothing else changed):
//   staging.hpp     errors, per-device constants, scratch pool, staging, host-path policy, duplex pipeline
//   capi_base.hip   management, primitive batch entries, shared helpers
//   capi_bash.hip   bashF, bashHash*
//   capi_belt.hip   belt block / CTR / MAC / modes / AEAD / belt-hash
//   capi_bign.hip   bign verification, validation, key generation, signing
//   capi_mixed.hip  bash + belt-MAC per message, ragged hash batches, path policy
//   capi_prg.hip    bash-prg (prg-hash, prg-ae) over ragged batches
//   capi_beltae.hip belt-dwp / belt-che over ragged batches of records
//   capi_fmt.hip    belt-fmt over batches of records, beltFMTEncr / beltFMTDecr
//   capi_kwp.hip    belt-kwp over batches of keys of one length
//   capi_hmac.hip   belt-hmac / belt-pbkdf2 over ragged batches, beltHMAC / beltPBKDF2
//   capi_bpki.hip   bpki password containers: PBKDF2 into a per-record-key belt-kwp, DER frames on the host
//   capi_exp.hip    experiment hooks (libbee2hip_exp.so only)
#include "staging.hpp"
static const bool g_capture_query_set = (bee2hip::g_stream_capturing = bee2hip::stream_is_capturing, true);
#include "capi_base.hip"
#include "capi_bash.hip"
#include "capi_belt.hip"
#include "capi_bign.hip"
#include "capi_mixed.hip"
#include "capi_prg.hip"
#include "capi_beltae.hip"
#include "capi_fmt.hip"
#include "capi_kwp.hip"
#include "capi_hmac.hip"
#include "capi_bpki.hip"
#include "capi_exp.hip"
