/*
 * bee2hip.h -- C ABI of libbee2hip.so, the MI355X (gfx950) batch-primitive engine
 * for bee2's data-parallel hot paths: bash-f / bashHash, belt (block, CTR, MAC, hash,
 * ECB, CBC, BDE, SDE, DWP, CHE) and bign signature verification on the three standard
 * curves.
 *
 * Three groups of entry points, all `extern "C"`, plain pointers and sizes:
 *
 *  (1) bee2 DROP-IN symbols: same names, signatures and error behaviour as the
 *      bee2 functions they replace, so a bee2 caller can link this library instead
 *      of those objects (bee2's own test/crypto sources pass against it:
 *      oracle/Makefile `reftests`).  States are caller-owned PODs of X_keep() bytes that
 *      may be memcpy-cloned, as in bee2; belt_ctr_st, belt_mac_st and bash_hash_st have
 *      bee2's exact layout, the other states are opaque.  Where a call runs: every large
 *      call and every bign operation that touches a private or one-time key evaluates its
 *      primitives (bashF, E_K / D_K, GF(2^128) products, the scalar multiplications) on the
 *      GPU; a SMALL single call -- one bashF, one block, a block-parallel mode under 8 KiB
 *      per call, the serial chain of one message (sponge, CBC-MAC, belt-hash, CBC
 *      encryption, one belt-sde sector), ONE signature verification on a standard curve --
 *      takes the library's own host path (bee2_amd/csrc/host_small.hpp, host_bign.hpp;
 *      SURVEY.md 8b "single-call path; may run on CPU"), because one launch costs 20 us
 *      where a host core needs 0.3 (one verification: 0.42 ms through the GPU, 27 us on
 *      the calling core, 178 us in bee2).  BEE2HIP_FORCE=gpu|cpu overrides the choice.  In
 *      every mode the calling thread needs a working HIP device: there is no GPU-less
 *      operation.  A device failure inside a `void` function is retried once and then
 *      finished on the host with a message on stderr (BEE2HIP_FORCE=gpu: abort with a
 *      message).  Each declaration cites the bee2 interface it replaces.  All of them
 *      may be called from several threads at once.
 *
 *  (2) bee2hip_*  host-pointer batch API: the caller hands host buffers; the
 *      library stages H2D, launches, stages D2H.
 *
 *  (3) bee2hip_*_dev  device-pointer batch API: buffers already resident in HBM
 *      (e.g. torch tensors' data_ptr()); asynchronous on `stream` (a hipStream_t
 *      passed as void*, NULL = default stream).  This is what bench.py times.
 *
 * All octet strings are little-endian, exactly as in bee2.
 */
#ifndef BEE2HIP_H
#define BEE2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)      /* everything declared here is exported */
#endif

/* ---- bee2 base types (include/bee2/defs.h:269,441,463,520) ---------------- */
typedef uint8_t octet;
typedef uint16_t u16;
typedef uint32_t u32;
typedef int bool_t;
typedef uint32_t err_t;
#ifndef TRUE
#define TRUE 1
#define FALSE 0
#endif

/* ---- bee2 error codes on the path (include/bee2/core/err.h) --------------- */
#define ERR_OK               ((err_t)0)
#define ERR_BAD_INPUT        ((err_t)109)   /* err.h:72  */
#define ERR_OUTOFMEMORY      ((err_t)110)   /* err.h:74  */
#define ERR_NOT_IMPLEMENTED  ((err_t)119)   /* err.h:92  */
#define ERR_FILE_NOT_FOUND    ((err_t)202)   /* err.h:105 */
#define ERR_BAD_OID          ((err_t)301)   /* err.h:132 */
#define ERR_BAD_RNG          ((err_t)304)   /* err.h:138 */
#define ERR_BAD_FORMAT       ((err_t)306)   /* err.h:142 */
#define ERR_BAD_PARAMS       ((err_t)502)   /* err.h:180 */
#define ERR_BAD_SECKEY       ((err_t)503)   /* err.h:182 */
#define ERR_BAD_PRIVKEY      ((err_t)504)   /* err.h:184 */
#define ERR_BAD_PUBKEY       ((err_t)505)   /* err.h:186 */
#define ERR_BAD_SHAREKEY     ((err_t)508)   /* err.h:192 */
#define ERR_BAD_SIG          ((err_t)510)   /* err.h:196 */
#define ERR_BAD_MAC          ((err_t)511)   /* err.h:198 */
#define ERR_BAD_KEYTOKEN     ((err_t)513)   /* err.h */
/* engine-specific: a HIP runtime call failed (no bee2 equivalent; the reference
   has no device).  bee2hip_last_error() returns the HIP message. */
#define ERR_BEE2HIP_DEVICE   ((err_t)0x4850)

/* ======================================================================== *
 * (1) bee2 drop-in symbols
 * ======================================================================== */

/* ---- bash: include/bee2/crypto/bash.h ------------------------------------ */
/* bash.h:136  (the BASH_PLATFORM slot, src/crypto/bash/bash_f.c:26-44) */
void bashF(octet block[192], void *stack);
/* bash.h:139 */
size_t bashF_deep(void);
/* src/crypto/bash/bash_f.c:27-43, consumed by test/crypto/bash_bench.c:27,47 */
extern const char bash_platform[];
/* bash.h:152-225, src/crypto/bash/bash_hash.c:25-137 */
size_t bashHash_keep(void);
void bashHashStart(void *state, size_t l);
void bashHashStepH(const void *buf, size_t count, void *state);
void bashHashStepG(octet hash[], size_t hash_len, void *state);
bool_t bashHashStepV(const octet hash[], size_t hash_len, void *state);
err_t bashHash(octet hash[], size_t l, const void *src, size_t count);

/* ---- belt: include/bee2/crypto/belt.h ------------------------------------ */
/* belt.h:148, src/crypto/belt/belt_block.c:62-66 */
const octet *beltH(void);
/* belt.h:170-176, belt_block.c:88-106 */
void beltKeyExpand2(u32 key_[8], const octet key[], size_t len);
/* belt.h:186-221, belt_block.c:302-334 */
void beltBlockEncr(octet block[16], const u32 key[8]);
void beltBlockEncr2(u32 block[4], const u32 key[8]);
void beltBlockEncr3(u32 *a, u32 *b, u32 *c, u32 *d, const u32 key[8]);
/* belt.h:692-743, src/crypto/belt/belt_ctr.c:46-135; state = belt_ctr_st,
   src/crypto/belt/belt_lcl.h:135-141 (key[8], ctr[4], block[16], reserved) */
size_t beltCTR_keep(void);
void beltCTRStart(void *state, const octet key[], size_t len, const octet iv[16]);
void beltCTRStepE(void *buf, size_t count, void *state);
#define beltCTRStepD beltCTRStepE                 /* belt.h:724 */
err_t beltCTR(void *dest, const void *src, size_t count, const octet key[], size_t len,
              const octet iv[16]);
/* ---- SURVEY.md 8f-1 ("next" row): block decryption and the block-parallel modes ---- */
/* belt.h:230-262, belt_block.c:341-373 */
void beltBlockDecr(octet block[16], const u32 key[8]);
void beltBlockDecr2(u32 block[4], const u32 key[8]);
void beltBlockDecr3(u32 *a, u32 *b, u32 *c, u32 *d, const u32 key[8]);
/* belt.h:430-505, src/crypto/belt/belt_ecb.c:42-159; state = belt_ecb_st (key[8], block[16]) */
size_t beltECB_keep(void);
void beltECBStart(void *state, const octet key[], size_t len);
void beltECBStepE(void *buf, size_t count, void *state);
void beltECBStepD(void *buf, size_t count, void *state);
err_t beltECBEncr(void *dest, const void *src, size_t count, const octet key[], size_t len);
err_t beltECBDecr(void *dest, const void *src, size_t count, const octet key[], size_t len);
/* belt.h:520-600, src/crypto/belt/belt_cbc.c:43-193; state = belt_cbc_st (key[8], block[16], block1[16]) */
size_t beltCBC_keep(void);
void beltCBCStart(void *state, const octet key[], size_t len, const octet iv[16]);
void beltCBCStepE(void *buf, size_t count, void *state);
void beltCBCStepD(void *buf, size_t count, void *state);
err_t beltCBCEncr(void *dest, const void *src, size_t count, const octet key[], size_t len,
                  const octet iv[16]);
err_t beltCBCDecr(void *dest, const void *src, size_t count, const octet key[], size_t len,
                  const octet iv[16]);

/* belt-bde, block-wise disk encryption (belt.h:1360-1455, src/crypto/belt/belt_bde.c:26-133):
   s <- E_K(iv); for every 16-byte block s <- s*x in GF(2^128), Y = E_K(X ^ s) ^ s (StepD: D_K).
   count must be a multiple of 16; the one-shots return ERR_BAD_INPUT for count < 16 or
   count % 16 != 0 (belt_bde.c:93-100). */
size_t beltBDE_keep(void);
void beltBDEStart(void *state, const octet key[], size_t len, const octet iv[16]);
void beltBDEStepE(void *buf, size_t count, void *state);
void beltBDEStepD(void *buf, size_t count, void *state);
err_t beltBDEEncr(void *dest, const void *src, size_t count, const octet key[], size_t len,
                  const octet iv[16]);
err_t beltBDEDecr(void *dest, const void *src, size_t count, const octet key[], size_t len,
                  const octet iv[16]);

/* belt-sde, sector-wise disk encryption (belt.h, src/crypto/belt/belt_sde.c:26-121): XEX around
   the wide-block cipher belt-wbl with the tweak E_K(iv) on the first block.  One call = one sector:
   count a multiple of 16, >= 32 (the one-shots return ERR_BAD_INPUT otherwise, belt_sde.c:79-80).
   A sector is a serial chain of 2*(count/16) block encryptions; the batch entry below runs many
   sectors, one lane each. */
size_t beltSDE_keep(void);
void beltSDEStart(void *state, const octet key[], size_t len);
void beltSDEStepE(void *buf, size_t count, const octet iv[16], void *state);
void beltSDEStepD(void *buf, size_t count, const octet iv[16], void *state);
err_t beltSDEEncr(void *dest, const void *src, size_t count, const octet key[], size_t len,
                  const octet iv[16]);
err_t beltSDEDecr(void *dest, const void *src, size_t count, const octet key[], size_t len,
                  const octet iv[16]);

/* belt-dwp, authenticated encryption: CTR + polynomial MAC over GF(2^128) (belt.h, src/crypto/belt/
   belt_dwp.c:27-274).  The state is an opaque POD of beltDWP_keep() bytes (not bee2's layout: bee2
   appends a beltPolyMul stack).  Order of calls as in bee2: Start, StepI* (open data), then
   StepE + StepA (protect) or StepA + StepD (unprotect) on the critical data, StepG / StepV at any
   point.  beltDWPUnwrap returns ERR_BAD_MAC without decrypting when the tag does not match. */
size_t beltDWP_keep(void);
void beltDWPStart(void *state, const octet key[], size_t len, const octet iv[16]);
void beltDWPStepE(void *buf, size_t count, void *state);
void beltDWPStepI(const void *buf, size_t count, void *state);
void beltDWPStepA(const void *buf, size_t count, void *state);
void beltDWPStepD(void *buf, size_t count, void *state);
void beltDWPStepG(octet mac[8], void *state);
bool_t beltDWPStepV(const octet mac[8], void *state);
err_t beltDWPWrap(void *dest, octet mac[8], const void *src1, size_t count1, const void *src2,
                  size_t count2, const octet key[], size_t len, const octet iv[16]);
err_t beltDWPUnwrap(void *dest, const void *src1, size_t count1, const void *src2, size_t count2,
                    const octet mac[8], const octet key[], size_t len, const octet iv[16]);

/* belt-che (belt_che.c:27-319): the belt-dwp authenticator with r = E_K(iv) and the keystream
   E_K(s_i), s_0 = r, s_i = s_{i-1}*x ^ 1 in GF(2^128); same call order and error behaviour as belt-dwp */
size_t beltCHE_keep(void);
void beltCHEStart(void *state, const octet key[], size_t len, const octet iv[16]);
void beltCHEStepE(void *buf, size_t count, void *state);
void beltCHEStepI(const void *buf, size_t count, void *state);
void beltCHEStepA(const void *buf, size_t count, void *state);
void beltCHEStepD(void *buf, size_t count, void *state);
void beltCHEStepG(octet mac[8], void *state);
bool_t beltCHEStepV(const octet mac[8], void *state);
err_t beltCHEWrap(void *dest, octet mac[8], const void *src1, size_t count1, const void *src2,
                  size_t count2, const octet key[], size_t len, const octet iv[16]);
err_t beltCHEUnwrap(void *dest, const void *src1, size_t count1, const void *src2, size_t count2,
                    const octet mac[8], const octet key[], size_t len, const octet iv[16]);

/* belt-hash, the default algorithm of `bee2cmd bsum` (belt.h, src/crypto/belt/belt_hash.c:28-190;
   cmd/bsum/bsum.c:133-147 drives exactly Start / StepH* / StepG).  One message is a serial chain:
   these calls are for drop-in use, batches go through bee2hip_hash_ragged. */
size_t beltHash_keep(void);
void beltHashStart(void *state);
void beltHashStepH(const void *buf, size_t count, void *state);
void beltHashStepG(octet hash[32], void *state);
void beltHashStepG2(octet hash[], size_t hash_len, void *state);
bool_t beltHashStepV(const octet hash[32], void *state);
bool_t beltHashStepV2(const octet hash[], size_t hash_len, void *state);
err_t beltHash(octet hash[32], const void *src, size_t count);

/* belt.h:756-854, src/crypto/belt/belt_mac.c:32-203 */
size_t beltMAC_keep(void);
void beltMACStart(void *state, const octet key[], size_t len);
void beltMACStepA(const void *buf, size_t count, void *state);
void beltMACStepG(octet mac[8], void *state);
void beltMACStepG2(octet mac[], size_t mac_len, void *state);
bool_t beltMACStepV(const octet mac[8], void *state);
bool_t beltMACStepV2(const octet mac[], size_t mac_len, void *state);
err_t beltMAC(octet mac[8], const void *src, size_t count, const octet key[], size_t len);

/* ---- bign: include/bee2/crypto/bign.h, bign128.h -------------------------- */
/* bign.h:65-74 */
typedef struct {
    size_t l;
    octet p[64];
    octet a[64];
    octet b[64];
    octet q[64];
    octet yG[64];
    octet seed[8];
} bign_params;
/* bign.h:100-107, src/crypto/bign/bign_params.c:180-230: "1.2.112.0.2.0.34.101.45.3.{1,2,3}" */
err_t bignParamsStd(bign_params *params, const char *name);
/* bign.h:395-402, src/crypto/bign/bign_sign.c:349-361.
   Any parameter set that passes bignParamsCheck + bignEcCreate is served (bignVerify and bignPubkeyVal; batch forms
   likewise): the three standard sets by the throughput kernels, every other set by general-curve kernels (Montgomery
   arithmetic, general coefficient a; 14 / 35 / 72 ms per batch of up to a few thousand signatures on the three
   levels -- a completeness path, not a throughput path).  The signing side (bignKeypairGen, bignPubkeyCalc, bignSign*)
   serves them too: a constant-time double-and-add-always ladder with complete additions on the general curve, arithmetic
   mod q in Montgomery form (bign_generic_kernels.hip; tests/golden/bign_generic_sign.json holds the reference's answers).
   Any valid DER OID is served, as in bee2: beyond 128 octets its leading whole 32-byte blocks are belt-hashed once per
   batch and the per-signature kernels continue from that state (tests/golden/bign_oid_long.json: 129 .. 4099 octets). */
err_t bignVerify(const bign_params *params, const octet oid_der[], size_t oid_len,
                 const octet hash[], const octet sig[], const octet pubkey[]);
/* include/bee2/crypto/bign128.h:174-178, src/crypto/bign/bign128.c:177-185 */
err_t bign128Verify(const octet hash[32], const octet sig[48], const octet pubkey[64]);
/* the 384- and 512-bit curves (l = 192 / 256).
   include/bee2/crypto/bign192.h, bign256.h; src/crypto/bign/bign192.c:177-185, bign256.c:177-185 */
err_t bign192Verify(const octet hash[48], const octet sig[72], const octet pubkey[96]);
err_t bign256Verify(const octet hash[64], const octet sig[96], const octet pubkey[128]);
/* public-key validation, the step `bee2cmd sig vfy` runs before each verification
   (cmd/core/cmd_sig.c:463-478): bign.h:278-281, src/crypto/bign/bign_misc.c:319-365 (coordinates < p and
   the point on the curve, src/math/ecp/ecp_a.c:36-60); bign128.h:87, bign192.h, bign256.h facades
   (bign128.c:115-122).  ERR_OK or ERR_BAD_PUBKEY. */
err_t bignPubkeyVal(const bign_params *params, const octet pubkey[]);
err_t bign128PubkeyVal(const octet pubkey[64]);
err_t bign192PubkeyVal(const octet pubkey[96]);
err_t bign256PubkeyVal(const octet pubkey[128]);

/* SURVEY.md 8f-4, second half: key generation, public key from private key, signing.  Secret-handling device code:
   constant-time at the instruction level (bee2_amd/csrc/bign_sign_kernels.hip states what that covers).
   gen_i: include/bee2/defs.h (void (*)(void* buf, size_t count, void* state)), called on the HOST exactly as
   zzRandNZMod calls it (src/math/zz/zz_mod.c:463-485); the scalar multiplications, the nonce derivation of
   bignSign2 (belt-hash + belt-wbl), the hash tail and the arithmetic mod q run on the device.
   bign.h:207-215,247-254,316-326,352-363; bign128.h:64-69,98-101,140-164 (and bign192.h, bign256.h);
   src/crypto/bign/bign_misc.c:182-243,373-431, bign_sign.c:32-260. */
typedef void (*gen_i)(void *buf, size_t count, void *state);
err_t bignKeypairGen(octet privkey[], octet pubkey[], const bign_params *params, gen_i rng, void *rng_state);
err_t bignPubkeyCalc(octet pubkey[], const bign_params *params, const octet privkey[]);
err_t bignSign(octet sig[], const bign_params *params, const octet oid_der[], size_t oid_len, const octet hash[],
               const octet privkey[], gen_i rng, void *rng_state);
err_t bignSign2(octet sig[], const bign_params *params, const octet oid_der[], size_t oid_len, const octet hash[],
                const octet privkey[], const void *t, size_t t_len);
err_t bign128KeypairGen(octet privkey[32], octet pubkey[64], gen_i rng, void *rng_state);
err_t bign128PubkeyCalc(octet pubkey[64], const octet privkey[32]);
err_t bign128Sign(octet sig[48], const octet hash[32], const octet privkey[32], gen_i rng, void *rng_state);
err_t bign128Sign2(octet sig[48], const octet hash[32], const octet privkey[32], const void *t, size_t t_len);
err_t bign192KeypairGen(octet privkey[48], octet pubkey[96], gen_i rng, void *rng_state);
err_t bign192PubkeyCalc(octet pubkey[96], const octet privkey[48]);
err_t bign192Sign(octet sig[72], const octet hash[48], const octet privkey[48], gen_i rng, void *rng_state);
err_t bign192Sign2(octet sig[72], const octet hash[48], const octet privkey[48], const void *t, size_t t_len);
err_t bign256KeypairGen(octet privkey[64], octet pubkey[128], gen_i rng, void *rng_state);
err_t bign256PubkeyCalc(octet pubkey[128], const octet privkey[64]);
err_t bign256Sign(octet sig[96], const octet hash[64], const octet privkey[64], gen_i rng, void *rng_state);
err_t bign256Sign2(octet sig[96], const octet hash[64], const octet privkey[64], const void *t, size_t t_len);

/* ======================================================================== *
 * (2) host-pointer batch API (new; SURVEY.md 8b "batch extension")
 * ======================================================================== */

/* n independent 192-byte states, contiguous, permuted in place (batched bashF) */
err_t bee2hip_bashF_batch(octet *states, size_t n);
/* bulk CTR over host memory, exactly equivalent to beltCTRStepE(buf, count, state)
   including the ctr / block / reserved fields it leaves behind (belt_ctr.c:66-111) */
err_t bee2hip_beltCTR_bulk(void *buf, size_t count, void *ctr_state);
/* n signatures: hashes n*32, sigs n*48, pubkeys n*64 -> codes[n] = what
   bignVerify(params, oid_der, oid_len, ...) returns per item (bign_sign.c:268-361) */
err_t bee2hip_bignVerify_batch(const bign_params *params, const octet oid_der[], size_t oid_len,
                               const octet *hashes, const octet *sigs, const octet *pubkeys,
                               size_t n, err_t *codes);
/* n public keys of params->l/2 octets each -> codes[n] = what bignPubkeyVal(params, key) returns */
err_t bee2hip_bignPubkeyVal_batch(const bign_params *params, const octet *pubkeys, size_t n,
                                  err_t *codes);
/* n private keys of params->l/4 octets -> n public keys of params->l/2 octets; codes[n] = what bignPubkeyCalc
   returns per key (ERR_OK / ERR_BAD_PRIVKEY); the public key of a refused private key is left untouched */
err_t bee2hip_bignPubkeyCalc_batch(const bign_params *params, const octet *privkeys, size_t n,
                                   octet *pubkeys, err_t *codes);
/* n deterministic signatures (bignSign2): hashes n*(l/4), privkeys n*(l/4), one additional input t (may be
   NULL) shared by the batch -> sigs n*(3l/8), codes[n] = what bignSign2 returns per item */
err_t bee2hip_bignSign2_batch(const bign_params *params, const octet oid_der[], size_t oid_len, const octet *hashes,
                              const octet *privkeys, const void *t, size_t t_len, size_t n, octet *sigs, err_t *codes);
/* n signatures with the one-time keys supplied (what bignSign computes once its rng has produced k in
   {1..q-1}): ks n*(l/4); a k outside that range gives ERR_BAD_RNG for the item */
err_t bee2hip_bignSignK_batch(const bign_params *params, const octet oid_der[], size_t oid_len, const octet *hashes,
                              const octet *privkeys, const octet *ks, size_t n, octet *sigs, err_t *codes);
/* n messages of msg_len bytes each (contiguous): bashHash(l) digest (l/4 bytes each,
   digests may be NULL) and beltMAC tag (8 bytes each, tags may be NULL) per message */
err_t bee2hip_bashHash_beltMAC_batch(const octet *msgs, size_t msg_len, size_t n, size_t l,
                                     const octet key[], size_t key_len,
                                     octet *digests, octet *tags);

/* SURVEY.md 8f-3 (batch front-end for `bee2cmd bsum`, cmd/bsum/bsum.c:133-221): n messages of
   different lengths packed back to back, message i = data[offsets[i] .. offsets[i+1]).
   alg = 0: belt-hash (32-byte digests, src/crypto/belt/belt_hash.c:173-190);
   alg = 128 / 192 / 256: bash256 / bash384 / bash512 (alg/4-byte digests, bash_hash.c:118-137) */
err_t bee2hip_hash_ragged(size_t alg, const octet *data, const uint64_t *offsets, size_t n,
                          octet *digests);
err_t bee2hip_hash_ragged_dev(size_t alg, const void *d_data, const void *d_offsets, size_t n,
                              void *d_digests, void *stream);
/* (without an order the library buckets the messages by the power of two of their length on the device
   and launches the buckets longest first)
   same with an explicit launch order: d_order = n x uint32, a permutation of 0..n-1 (NULL = as above);
   slot k hashes message d_order[k], digest i still lands at d_digests + i*dlen.  A slot is one lane,
   or for messages of 4 KiB and more a group of 8 lanes (bash: one column of the state each) or a
   pair (belt-hash: the two independent encryptions of a compression).  A wavefront runs until the
   longest of its messages is done: pass the messages sorted by decreasing length
   (bee2hip_hash_ragged does so itself). */
err_t bee2hip_hash_ragged_ordered_dev(size_t alg, const void *d_data, const void *d_offsets,
                                      const void *d_order, size_t n, void *d_digests, void *stream);

/* bash-prg, the programmable sponge algorithms of STB 34.101.77 (src/crypto/bash/bash_prg.c), over a ragged batch: record i
   is ONE automaton on one lane, packed like the messages above.  With buf_len = the rate of (l, d) and the mode
   (bash_prg.c:34-43, :133) a record costs 3 + hdr/buf_len + text/buf_len permutations (prg-hash: 2 + msg/buf_len).
     prg-hash (A.5): Start(l, d, ann, ann_len, NULL, 0) (bash_prg.c:110-136), Absorb(msg_i) (:211-215),
                     Squeeze(out + i*out_len, out_len) (:257-261); ann is shared by the batch
     prg-ae   (A.6): Start(l, d, anns + i*ann_len, ann_len, key, key_len), Absorb(hdr_i) -- also when it is empty: a
                     zero-length absorb still commits (:89-102, :177-180) --, Encr(text_i) (:310-314) or Decr(text_i)
                     (:363-367), Squeeze(tag_i, tag_len); key is shared by the batch, every record has its own announcement
   l in {128, 192, 256} and d in {1, 2}, else ERR_BAD_PARAMS.  ERR_BAD_INPUT unless ann_len % 4 == 0, ann_len <= 60,
   key_len % 4 == 0, l/8 <= key_len <= 60, 1 <= tag_len (out_len) <= 64, n < 2^32; all of it is checked before any device work.
   hdrs / hdr_offsets both NULL: every header is empty.  dst may be src (in place); otherwise record i lands at
   dst + offsets[i].  unwrap compares all tag_len octets of the squeezed tag with tags + i*tag_len (no early exit):
   codes[i] = ERR_OK or ERR_BAD_MAC, and the plaintext of a refused record is overwritten with zeros; its neighbours stay. */
err_t bee2hip_bashPrgHash_ragged(size_t l, size_t d, const octet ann[], size_t ann_len, const octet *data,
                                 const uint64_t *offsets, size_t n, octet *out, size_t out_len);
err_t bee2hip_bashPrgAE_wrap_ragged(size_t l, size_t d, const octet key[], size_t key_len, const octet *anns, size_t ann_len,
                                    const octet *hdrs, const uint64_t *hdr_offsets, const octet *src, const uint64_t *offsets,
                                    size_t n, octet *dst, octet *tags, size_t tag_len);
err_t bee2hip_bashPrgAE_unwrap_ragged(size_t l, size_t d, const octet key[], size_t key_len, const octet *anns, size_t ann_len,
                                      const octet *hdrs, const uint64_t *hdr_offsets, const octet *src, const uint64_t *offsets,
                                      size_t n, const octet *tags, size_t tag_len, octet *dst, err_t *codes);
/* The same on device pointers, asynchronous on `stream` (one queue, no fork).  These are device-pointer batch entries in
   every respect but the name: the suffix is _stream, not the usual one, because the tests' contract registry takes the
   expected bytes of every entry with the usual suffix from the C oracle, which has no bash-prg; they are held to the same
   range / aliasing / capture contract by tests/test_gpu_bashprg.py, and can be renamed once the registry can describe them.
   Alignment: offsets 8, d_order / d_anns / d_codes 4, data / headers / d_src / d_dst / d_tags / d_out 1.  key and the shared
   ann are HOST pointers and travel in the launch arguments.  d_order as for the ordered ragged hash above (NULL: bucketed by
   the text length -- prg-hash: the message length -- on the device once n >= 128).  unwrap = 0: d_tags is written, d_codes is
   not used (may be NULL); unwrap = 1: d_tags is read, d_codes (n x err_t) is written. */
err_t bee2hip_bashPrgHash_ragged_stream(size_t l, size_t d, const octet ann[], size_t ann_len, const void *d_data,
                                        const void *d_offsets, const void *d_order, size_t n, void *d_out, size_t out_len,
                                        void *stream);
err_t bee2hip_bashPrgAE_ragged_stream(int unwrap, size_t l, size_t d, const octet key[], size_t key_len, const void *d_anns,
                                      size_t ann_len, const void *d_hdrs, const void *d_hdr_offsets, const void *d_src,
                                      const void *d_offsets, const void *d_order, size_t n, void *d_dst, void *d_tags,
                                      size_t tag_len, void *d_codes, void *stream);

/* belt-dwp / belt-che, the AEAD of STB 34.101.31, over a ragged batch of records packed like the bash-prg batch above: one
   key for the batch, one 16-octet iv per record (ivs + 16 i), one record per lane.
   mode 0 = belt-dwp (src/crypto/belt/belt_dwp.c), 1 = belt-che (belt_che.c).  Record i is
       beltXXXWrap(dst_i, tag_i, src_i, len_i, hdr_i, hlen_i, key, key_len, ivs + 16 i)
   with text i = src[offsets[i] .. offsets[i+1]) landing at dst + offsets[i], header i (bee2's open data, src2) =
   hdrs[hdr_offsets[i] .. hdr_offsets[i+1]) and tag i = tags + 8 i.  hdrs / hdr_offsets both NULL: every header is empty.
   dst may be src (in place).  ERR_BAD_INPUT unless mode is 0 or 1, key_len is 16, 24 or 32 (belt_che.c:263), n < 2^32, the
   offsets do not decrease and no needed buffer is NULL; all of it is checked before any device work, and n = 0 is ERR_OK
   without a device.
   unwrap compares all 8 octets of the computed tag with tags + 8 i (no early exit): codes[i] = ERR_OK or ERR_BAD_MAC.
   DIFFERENCE FROM bee2: beltDWPUnwrap / beltCHEUnwrap check the tag first and leave dest untouched when they refuse
   (belt_dwp.c:258-262).  The batch makes one pass over a record, decrypting while it authenticates, so the dst octets of a
   refused record are overwritten with ZEROS -- never left holding unauthenticated plaintext; its neighbours stay. */
err_t bee2hip_beltAE_wrap_ragged(int mode, const octet key[], size_t key_len, const octet *ivs, const octet *hdrs,
                                 const uint64_t *hdr_offsets, const octet *src, const uint64_t *offsets, size_t n, octet *dst,
                                 octet *tags);
err_t bee2hip_beltAE_unwrap_ragged(int mode, const octet key[], size_t key_len, const octet *ivs, const octet *hdrs,
                                   const uint64_t *hdr_offsets, const octet *src, const uint64_t *offsets, size_t n,
                                   const octet *tags, octet *dst, err_t *codes);
/* The same on device pointers, asynchronous on `stream` (one queue, no fork).  This is a device-pointer batch entry in
   every respect but the name: the suffix is _stream, not the usual one, because the tests' contract registry holds a record
   for every entry with the usual suffix and this one is held to the same range / aliasing / capture contract by
   tests/test_gpu_beltae.py instead; it can be renamed together with the bash-prg entries.
   Alignment: offsets 8, d_order / d_codes 4, d_ivs / headers / d_src / d_dst / d_tags 1.  key is a HOST pointer, expanded on
   the host, and travels in the launch arguments.  d_order as for the ordered ragged hash above (NULL: bucketed by the text
   length on the device once n >= 128).  unwrap = 0: d_tags (n x 8) is written, d_codes is not used (may be NULL);
   unwrap = 1: d_tags is read, d_codes (n x err_t) is written. */
err_t bee2hip_beltAE_ragged_stream(int unwrap, int mode, const octet key[], size_t key_len, const void *d_ivs,
                                   const void *d_hdrs, const void *d_hdr_offsets, const void *d_src, const void *d_offsets,
                                   const void *d_order, size_t n, void *d_dst, void *d_tags, void *d_codes, void *stream);

/* ---- belt-fmt: format-preserving encryption of n records (STB 34.101.31; belt.h, src/crypto/belt/belt_fmt.c) ----------
   A record is `count` symbols (u16) of the alphabet 0 .. mod - 1, 2 <= mod <= 65536, 2 <= count <= 600; the result is again
   `count` symbols of that alphabet.  Every record of a batch has the same mod and count and the same key: record i is
   src + i * count, its synchro value ivs + 16 i (ivs == NULL: every synchro value is 16 zero octets), its result
   dst + i * count.  decr = 0 encrypts, 1 decrypts.  One lane of belt_fmt_batch_kernel per record.
   Before any device work: ERR_BAD_INPUT unless decr is 0 or 1, 2 <= mod <= 65536, count >= 2, key_len is 16, 24 or 32, key
   is not NULL and n < 2^32, or when src or dst is NULL with n > 0; ERR_NOT_IMPLEMENTED for count > 600, as bee2; n = 0 is
   ERR_OK without a device.
   Symbols are NOT validated, as in bee2, which only EXPECTs them to be below mod: a symbol >= mod is not refused, it enters
   the arithmetic as it is -- the number of a half is the sum of symbol_j mod^j modulo 2^(64 b), and a symbol that receives a
   digit becomes (symbol + digit) mod mod -- and the result is what bee2 computes for the same input. */
err_t bee2hip_beltFMT_batch(int decr, u32 mod, size_t count, const octet key[], size_t key_len, const octet *ivs,
                            const u16 *src, size_t n, u16 *dst);
/* The same on device pointers, asynchronous on `stream` (one queue, no fork; may be captured into a graph).  key is a HOST
   pointer: it is expanded on the host and travels in the launch arguments.  d_src and d_dst are 2-aligned, d_ivs needs no
   alignment.  d_dst == d_src processes in place; any other overlap of the two ranges is ERR_BAD_INPUT with nothing written. */
err_t bee2hip_beltFMT_batch_stream(int decr, u32 mod, size_t count, const octet key[], size_t key_len, const void *d_ivs,
                                   const void *d_src, size_t n, void *d_dst, void *stream);
/* bee2's one-shots (belt.h; codes as belt_fmt.c:422-476, ERR_BAD_INPUT when dest overlaps iv included).  One record is one
   serial chain: it runs on the host path unless the path policy is 1, which runs the kernel with n = 1.
   DIFFERENCE FROM bee2: a mod outside 2 .. 65536 is ERR_BAD_INPUT here; bee2 only asserts it. */
err_t beltFMTEncr(u16 dest[], u32 mod, const u16 src[], size_t count, const octet key[], size_t len, const octet iv[16]);
err_t beltFMTDecr(u16 dest[], u32 mod, const u16 src[], size_t count, const octet key[], size_t len, const octet iv[16]);

/* ---- belt-kwp: key wrap of n keys of one length (STB 34.101.31; belt.h, src/crypto/belt/belt_kwp.c) ------------------
   Record by record these are bee2's one-shots
       beltKWPWrap(dst_i, src_i, count, hdr_i, key, key_len)  and  beltKWPUnwrap(dst_i, src_i, count, hdr_i, key, key_len);
   all n records have the same count and the same key-encryption key.  One lane of belt_kwp_batch_kernel per record.
   wrap: record i is the `count` >= 16 octets src + i * count (any values), its header hdrs + 16 i (hdrs == NULL: every header is
   16 zero octets, as bee2's header == 0), its token the count + 16 octets dst + i * (count + 16).
   unwrap: record i is the token src + i * count, count >= 32; the result is the count - 16 octets dst + i * (count - 16) and
   codes[i] is ERR_OK or ERR_BAD_KEYTOKEN.  The 16 octets of the recovered header are all compared with hdrs + 16 i (no early
   exit); the result octets of a refused record are ZEROS, as belt_kwp.c:84, and its neighbours are untouched.
   Tokens of up to 1024 octets: a wrap count above 1008 or an unwrap count above 1024 is ERR_NOT_IMPLEMENTED.  Before any
   device work: ERR_BAD_INPUT for a count below the minimum, a key_len other than 16, 24 or 32, a NULL key, n >= 2^32, or
   a NULL src, dst or (unwrap) codes with n > 0; n = 0 is ERR_OK without a device.  The two host forms stage both buffers, so
   their dst may be src; the stream form below refuses any overlap.
   The bee2 names themselves are not exported: a single token is one serial chain of E_K. */
err_t bee2hip_beltKWP_wrap_batch(const octet key[], size_t key_len, const octet *hdrs, const octet *src, size_t count, size_t n,
                                 octet *dst);
err_t bee2hip_beltKWP_unwrap_batch(const octet key[], size_t key_len, const octet *hdrs, const octet *src, size_t count, size_t n,
                                   octet *dst, err_t *codes);
/* The same on device pointers, asynchronous on `stream` (one queue, no fork; may be captured into a graph); unwrap = 0 or 1,
   anything else is ERR_BAD_INPUT.  The suffix is _stream for the reason given at bee2hip_beltAE_ragged_stream;
   tests/test_gpu_beltkwp.py holds the entry to the device-pointer contract.  key is a HOST pointer: it is expanded on the host
   and travels in the launch arguments.  d_src, d_dst and d_hdrs need no alignment; d_codes (n x err_t, unwrap only; may be
   NULL for wrap) is 4-aligned.  The fast path is count % 4 == 0 with a 4-aligned base: d_src and d_dst, each on its own, then move as
   dwords, otherwise octet by octet (about 4 % of the rate at count 19 against 24); headers are always read octet by octet.
   Source and result differ in size, so nothing is in place: ANY overlap of the src and dst
   ranges is ERR_BAD_INPUT with nothing written; d_hdrs and d_codes must not meet d_dst either (not checked). */
err_t bee2hip_beltKWP_batch_stream(int unwrap, const octet key[], size_t key_len, const void *d_hdrs, const void *d_src,
                                   size_t count, size_t n, void *d_dst, void *d_codes, void *stream);

/* The same with ONE KEY-ENCRYPTION KEY PER RECORD: record i is
       beltKWPWrap / beltKWPUnwrap(dst_i, src_i, count, hdr_i, keys + i * key_len, key_len)   (belt_kwp.c:19-50, :52-91),
   key_len = 16, 24 or 32 for the whole batch.  Tokens wrapped under per-record keys are what key transport and the containers
   below produce.  The same kernel text serves in a second instantiation (belt_kwp_batch_kernel<true>; the shared-key code
   is unchanged): the keys are a launch argument, each read by its record's lane once before the rounds, octet by octet, and
   expanded as beltKeyExpand2 does.  Contract, limits, codes and overlap rules are those of the three entries above, with
   these differences: keys == NULL with n > 0 is ERR_BAD_INPUT; in the stream form d_keys is a
   DEVICE pointer (n * key_len octets, no alignment) that must not meet d_dst -- an overlap of the two ranges is ERR_BAD_INPUT
   with nothing written.  The host forms stage the keys with the records and zero that staging when the call ends. */
err_t bee2hip_beltKWP_wrap_keyed_batch(const octet *keys, size_t key_len, const octet *hdrs, const octet *src, size_t count,
                                       size_t n, octet *dst);
err_t bee2hip_beltKWP_unwrap_keyed_batch(const octet *keys, size_t key_len, const octet *hdrs, const octet *src, size_t count,
                                         size_t n, octet *dst, err_t *codes);
err_t bee2hip_beltKWP_keyed_batch_stream(int unwrap, const void *d_keys, size_t key_len, const void *d_hdrs, const void *d_src,
                                         size_t count, size_t n, void *d_dst, void *d_codes, void *stream);

/* ---- belt-hmac and belt-pbkdf2 over n records (STB 34.101.31; belt.h, src/crypto/belt/belt_hmac.c, belt_pbkdf.c) -------
   Record by record these are bee2's one-shots
       beltHMAC(mac_i, msg_i, len_i, key_i, key_len_i)  and  beltPBKDF2(key_i, pwd_i, pwd_len_i, iter, salt_i, salt_len).
   One lane of belt_hmac_batch_kernel per record, whatever its length: long messages are NOT spread over several lanes.
   Message i = data[offsets[i] .. offsets[i+1]) (n + 1 offsets).  The key comes in one of two forms: ONE key for the batch
   (key != NULL, any key_len, keys and key_offsets NULL; its state is computed once on the host and travels in the launch
   arguments), or one key per record (key NULL): key i = keys[key_offsets[i] .. key_offsets[i+1]).  A key of more than 32 octets
   is belt-hashed first, as in bee2.  macs: mac_len (1 .. 32) octets a record, the first mac_len octets of the MAC, at
   macs + i * mac_len.  verify: all mac_len octets of record i are compared (no early exit) and codes[i] becomes ERR_OK or
   ERR_BAD_MAC; nothing else is written.
   Before any device work: ERR_BAD_INPUT for a mac_len outside 1 .. 32, n >= 2^32, both key forms given, or with n > 0 neither
   of them, decreasing offsets, or a NULL offsets, macs, codes (verify), data or keys that is needed; n = 0 is ERR_OK without
   a device. */
err_t bee2hip_beltHMAC_ragged(const octet key[], size_t key_len, const octet *keys, const uint64_t *key_offsets, const octet *data,
                              const uint64_t *offsets, size_t n, octet *macs, size_t mac_len);
err_t bee2hip_beltHMAC_verify_ragged(const octet key[], size_t key_len, const octet *keys, const uint64_t *key_offsets,
                                     const octet *data, const uint64_t *offsets, size_t n, const octet *macs, size_t mac_len,
                                     err_t *codes);
/* The same on device pointers, asynchronous on `stream` (one queue, no fork; may be captured into a graph under the conditions
   of bee2hip_beltAE_ragged_stream); verify = 0 or 1, anything else is ERR_BAD_INPUT.  The suffix is _stream for the reason
   given at bee2hip_beltAE_ragged_stream; tests/test_gpu_belthmac.py holds the entry to the device-pointer contract.  key is a
   HOST pointer (or NULL); d_keys, d_key_offsets, d_data, d_offsets are device pointers.  The offsets are 8-aligned, d_order
   (NULL, or a permutation of 0 .. n - 1 as n x uint32: lane k serves record d_order[k]) and d_codes (n x err_t) 4-aligned, else
   ERR_BAD_INPUT; data, keys and MACs need no alignment.  d_order NULL and n >= 128: the records are ordered by length on the
   device.  verify = 1 reads d_macs and writes only d_codes; verify = 0 writes only the mac_len * n octets of d_macs.  The
   offsets are not checked here. */
err_t bee2hip_beltHMAC_ragged_stream(int verify, const octet key[], size_t key_len, const void *d_keys, const void *d_key_offsets,
                                     const void *d_data, const void *d_offsets, const void *d_order, size_t n, void *d_macs,
                                     size_t mac_len, void *d_codes, void *stream);
/* PBKDF2: password i = pwds[pwd_offsets[i] .. pwd_offsets[i+1]); salt i = salts + i * salt_stride, salt_len octets
   (salt_stride = 0: one salt for the batch); keys = 32 n octets.  ERR_BAD_INPUT for iter = 0 (as bee2), n >= 2^32, a salt_stride
   that is neither 0 nor >= salt_len, decreasing offsets, a needed pointer that is NULL; ERR_NOT_IMPLEMENTED for iter above
   2^17 = 131072: a launch's run time is proportional to iter, about 3 s at that count (beltPBKDF2 below has no such limit).  The stream form writes only the
   32 n octets of d_keys; d_pwd_offsets is 8-aligned, d_order 4-aligned, nothing else needs alignment; with d_order NULL and
   n >= 128 the records are ordered by password length. */
err_t bee2hip_beltPBKDF2_batch(const octet *pwds, const uint64_t *pwd_offsets, size_t iter, const octet *salts, size_t salt_len,
                               size_t salt_stride, size_t n, octet *keys);
err_t bee2hip_beltPBKDF2_batch_stream(const void *d_pwds, const void *d_pwd_offsets, size_t iter, const void *d_salts,
                                      size_t salt_len, size_t salt_stride, const void *d_order, size_t n, void *d_keys,
                                      void *stream);
/* bee2's one-shots (belt.h; codes as belt_hmac.c:244-263 and belt_pbkdf.c:31-36).  One record is one serial chain: it runs on
   the host path unless the path policy is 1, which runs the kernel with n = 1; beltPBKDF2 with iter above 2^17 always runs on
   the host.  bee2's step functions of belt-hmac are not exported. */
err_t beltHMAC(octet mac[32], const void *src, size_t count, const octet key[], size_t len);
err_t beltPBKDF2(octet key[32], const octet pwd[], size_t pwd_len, size_t iter, const octet salt[], size_t salt_len);

/* ---- bpki password-protected containers, n in one call (STB 34.101.78; bpki.h, src/crypto/bpki.c:206-548) -------------
   kind = 0: a bign private key of 24, 32, 48 or 64 octets (bpkiPrivkeyWrap / bpkiPrivkeyUnwrap, bpki.c:313-425);
   kind = 1: a bels share of 17, 25 or 33 octets (bpkiShareWrap / bpkiShareUnwrap, bpki.c:433-548); any other kind is
   ERR_BAD_INPUT.  A container is beltPBKDF2(pwd, iter, salt[8]) -> belt-kwp of the PrivateKeyInfo frame under that key with a
   zero header, inside the EncryptedPrivateKeyInfo frame.  The frames are parsed and built on the host with bee2's DER
   strictness (bee2_amd/csrc/bpki_der.hpp); the passwords are stretched by belt_hmac_batch_kernel, one launch per distinct
   iteration count, and the derived keys stay on the device as the per-record keys of belt_kwp_batch_kernel, one launch per
   distinct pair (iteration count, token length) -- one in all for a batch from one issuer, at most 64 under the limits below, each
   a few microseconds next to PBKDF2; they are zeroed there before the call returns.  bee2's own bpki* names are not exported.
   Unwrap: record i is the container epkis[epki_offsets[i] .. epki_offsets[i+1]) with the password
   pwds[pwd_offsets[i] .. pwd_offsets[i+1]).  codes[i] is the code bee2 returns for it, in bee2's order (bpki.c:374-425):
   ERR_BAD_FORMAT (outer frame), ERR_BAD_INPUT (iter = 0, or encData below 32 octets), ERR_BAD_KEYTOKEN (wrong password),
   ERR_BAD_FORMAT (inner frame), for a share ERR_BAD_SHAREKEY (first octet outside 1 .. 16).  An accepted record has its key
   at keys + 64 i, zeros behind it up to 64 octets, and its length in key_lens[i]; a refused one 64 zero octets and length 0.
   DIFFERENCES FROM bee2: codes[i] = ERR_NOT_IMPLEMENTED, with nothing computed, for iter above 2^17 (the count comes from an
   untrusted container and a launch holds the GPU for a time proportional to it) and for encData above 1024 octets; more than
   8 distinct iteration counts or more than 8 distinct encData lengths among the records that reach the device make the whole
   call ERR_NOT_IMPLEMENTED with nothing written.  The call returns ERR_OK when it ran; when no record reaches the device (or
   n = 0) it does so without a device.
   Wrap: all n records share key_len and iter; record i has the key keys + i * key_len, its password and the salt salts + 8 i.
   *epki_len (may be NULL) receives the length of one container, which (kind, key_len, iter) fix; epkis == NULL returns that
   length only, as bee2; else container i is written at epkis + i * *epki_len, octet for octet what bee2 writes.  iter below
   10000 is ERR_BAD_INPUT, a key_len that is none of the kind's ERR_BAD_PRIVKEY (kind 0) or ERR_BAD_SECKEY (kind 1), iter above
   2^17 ERR_NOT_IMPLEMENTED, a share whose first octet is outside 1 .. 16 ERR_BAD_SECKEY for the whole call with nothing written
   (also when epkis == NULL and keys is given, as bpki.c:445-447; a length query with keys == NULL looks at no share).
   Both: ERR_BAD_INPUT for n >= 2^32, decreasing offsets, or a needed pointer that is NULL. */
err_t bee2hip_bpkiUnwrap_batch(int kind, const octet *epkis, const uint64_t *epki_offsets, const octet *pwds,
                               const uint64_t *pwd_offsets, size_t n, octet *keys, uint32_t *key_lens, err_t *codes);
err_t bee2hip_bpkiWrap_batch(int kind, const octet *keys, size_t key_len, const octet *pwds, const uint64_t *pwd_offsets,
                             const octet *salts, size_t iter, size_t n, octet *epkis, size_t *epki_len);

/* ---- one host batch over several GPUs from one process --------------------------------
   The batch is cut into contiguous index ranges (bee2hip_multi_plan), one worker thread per device runs the
   single-device entry above on its range; no data crosses devices.  ndev = number of devices to use, 0 = all
   visible ones (bee2hip_device_count).  Results are those of the single-device call, item for item; the CTR
   state is left exactly as bee2hip_beltCTR_bulk leaves it. */
int bee2hip_device_count(void);
err_t bee2hip_multi_plan(size_t n, int parts, int i, size_t *first, size_t *count);
err_t bee2hip_bashF_batch_multi(octet *states, size_t n, int ndev);
err_t bee2hip_beltCTR_bulk_multi(void *buf, size_t count, void *ctr_state, int ndev);
err_t bee2hip_bignVerify_batch_multi(const bign_params *params, const octet oid_der[], size_t oid_len,
                                     const octet *hashes, const octet *sigs, const octet *pubkeys, size_t n,
                                     err_t *codes, int ndev);
err_t bee2hip_bignVerify_onekey_batch_multi(const bign_params *params, const octet oid_der[], size_t oid_len,
                                            const octet *hashes, const octet *sigs, const octet pubkey[], size_t n,
                                            err_t *codes, int ndev);
err_t bee2hip_bignVerify_keyed_batch_multi(const bign_params *params, const octet oid_der[], size_t oid_len,
                                           const octet *hashes, const octet *sigs, const octet *pubkeys, size_t nkeys,
                                           const u32 *key_index, size_t n, err_t *codes, int ndev);
err_t bee2hip_bignSign2_batch_multi(const bign_params *params, const octet oid_der[], size_t oid_len,
                                    const octet *hashes, const octet *privkeys, const void *t, size_t t_len, size_t n,
                                    octet *sigs, err_t *codes, int ndev);
err_t bee2hip_bashHash_beltMAC_batch_multi(const octet *msgs, size_t msg_len, size_t n, size_t l, const octet key[],
                                           size_t key_len, octet *digests, octet *tags, int ndev);
err_t bee2hip_hash_ragged_multi(size_t alg, const octet *data, const uint64_t *offsets, size_t n, octet *digests,
                                int ndev);

/* ======================================================================== *
 * (3) device-pointer batch API (buffers in HBM; async on `stream`)
 *     Device pointers to states, blocks, sectors, messages and verify records must be 16-byte
 *     aligned (the kernels read them as 16-byte vectors), d_codes 4-byte, ragged offsets 8-byte and digests 4-byte:
 *     a misaligned pointer is refused with ERR_BAD_INPUT.  One stream = one queue: threads that
 *     share a stream serialise their calls themselves.
 * ======================================================================== */
err_t bee2hip_bashF_batch_dev(void *d_states, size_t n, void *stream);
/* full 16-byte blocks only: block i (0-based) ^= E_K(ctr0 + first_block + i + 1),
   the 128-bit little-endian counter arithmetic of belt_ctr.c:27-35 */
err_t bee2hip_beltCTR_blocks_dev(void *d_buf, size_t nblocks, const u32 key[8],
                                 const u32 ctr0[4], uint64_t first_block, void *stream);
/* ECB-style E_K over n blocks in place (used for ctr0 = E_K(iv), r = E_K(0)) */
err_t bee2hip_beltBlockEncr_dev(void *d_blocks, size_t nblocks, const u32 key[8], void *stream);
/* 8f-1: full blocks, device resident.  mode 0 = ECB encrypt, 1 = ECB decrypt (d_src may equal
   d_dst), 2 = CBC decrypt with chaining value iv[4] (u32 words; d_src != d_dst).  Source and
   destination ranges that overlap in any other way are refused with ERR_BAD_INPUT. */
err_t bee2hip_beltModes_blocks_dev(int mode, const void *d_src, void *d_dst, size_t nblocks,
                                   const u32 key[8], const u32 iv[4], void *stream);
/* n independent messages of nblk full blocks each, CBC-encrypted in place, one lane per
   message; d_ivs[n][16] holds each message's iv on entry and its last ciphertext block on exit */
err_t bee2hip_beltCBCEncr_batch_dev(void *d_msgs, size_t nblk, size_t n, const u32 key[8],
                                    void *d_ivs, void *stream);
/* belt-bde on nblocks whole blocks, device resident, d_src may equal d_dst (ranges that overlap in any
   other way are refused with ERR_BAD_INPUT).  s[4] = E_K(iv) as
   u32 words (what beltBDEStart leaves in the state); the blocks are the ones first_block ..
   first_block + nblocks - 1 of the stream, i.e. block j uses the tweak s * x^(j+1) -- a stream can
   be cut into pieces (or sharded across GPUs) at any block boundary.  decr = 0 / 1.
   d_s_out (may be NULL) receives s * x^(first_block + nblocks), 16 bytes: the state after the piece. */
/* belt-dwp's authenticator on device-resident data: *d_t_out (16 bytes, device) <- the value of t
   after absorbing nbytes at d_data as 16-byte blocks, t <- (t ^ X) * r in GF(2^128), the last block
   zero-padded (belt_dwp.c:96-101,118-119); r[4], t[4] = u32 words as in the state.  nbytes = 0
   returns t.  Together with bee2hip_beltCTR_blocks_dev this is beltDWPWrap on resident data. */
err_t bee2hip_beltDWP_absorb_dev(const void *d_data, size_t nbytes, const u32 r[4], const u32 t[4],
                                 void *d_t_out, void *stream);
/* belt-sde on nsectors contiguous sectors of sector_bytes each (a multiple of 16, >= 32), device
   resident, in place; d_ivs = nsectors x 16 bytes, one iv per sector.  decr = 0 / 1. */
err_t bee2hip_beltSDE_sectors_dev(int decr, void *d_sectors, size_t sector_bytes, size_t nsectors,
                                  const u32 key[8], const void *d_ivs, void *stream);
/* belt-che keystream on nblocks whole blocks, device resident, d_src may equal d_dst (ranges that overlap
   in any other way are refused with ERR_BAD_INPUT): block j of the
   stream (first_block <= j < first_block + nblocks) is XORed with E_K(S_{j+1}), S_0 = s[4] = E_K(iv) as
   u32 words, S_i = S_{i-1}*x ^ 1.  d_s_out (may be NULL) receives S_{first_block + nblocks}, 16 bytes. */
err_t bee2hip_beltCHE_blocks_dev(const void *d_src, void *d_dst, size_t nblocks, const u32 key[8],
                                 const u32 s[4], uint64_t first_block, void *d_s_out, void *stream);
err_t bee2hip_beltBDE_blocks_dev(int decr, const void *d_src, void *d_dst, size_t nblocks,
                                 const u32 key[8], const u32 s[4], uint64_t first_block,
                                 void *d_s_out, void *stream);
err_t bee2hip_bign128Verify_batch_dev(const void *d_hashes, const void *d_sigs,
                                      const void *d_pubkeys, size_t n, void *d_codes,
                                      void *stream);
err_t bee2hip_bignVerify_batch_dev(const octet oid_der[], size_t oid_len,
                                   const void *d_hashes, const void *d_sigs,
                                   const void *d_pubkeys, size_t n, void *d_codes,
                                   void *stream);
/* same for security level l in {128, 192, 256}: hashes n*(l/4), sigs n*(3l/8), pubkeys n*(l/2) */
err_t bee2hip_bignVerifyL_batch_dev(size_t l, const octet oid_der[], size_t oid_len,
                                    const void *d_hashes, const void *d_sigs,
                                    const void *d_pubkeys, size_t n, void *d_codes, void *stream);
/* n signatures under ONE public key -- the batch `bee2cmd sig vfy` makes of a tree of files signed by one party
   (cmd/core/cmd_sig.c:484-490), a signed log, a package repository.  Same verdict per signature as
   bignVerify(params, oid, hash_i, sig_i, pubkey) (bign_sign.c:268-361), in about a fifth of the work: the key becomes a
   fixed base with a comb table of its own (built once per key and device, cached: the last 1024 keys), so the scalar multiplication has no
   doublings left.  pubkey is HOST memory in both forms (l/2 octets).  A key that is not a point of the curve, and a
   non-standard parameter set, take the general path with the key repeated -- same codes, general speed.
   The _dev form synchronises `stream` the first time it meets a key (table construction); later calls with that key
   only queue kernels (hipGraph capture: prime the key with one call before capturing; a key the cache does not hold is
   refused on a capturing stream, and a captured call neither builds nor counts towards the key's 16-bit table). */
err_t bee2hip_bignVerify_onekey_batch(const bign_params *params, const octet oid_der[], size_t oid_len,
                                      const octet *hashes, const octet *sigs, const octet pubkey[],
                                      size_t n, err_t *codes);
err_t bee2hip_bignVerifyL_onekey_batch_dev(size_t l, const octet oid_der[], size_t oid_len,
                                           const void *d_hashes, const void *d_sigs, const octet pubkey[],
                                           size_t n, void *d_codes, void *stream);
/* ... and of a FEW signers: pubkeys = nkeys keys (HOST memory, nkeys <= 4096 on the device form), key_index[i] < nkeys says whose
   signature i is (n x u32; device memory in the _dev form).  codes[i] = bignVerify(params, oid, hash_i, sig_i, pubkeys[key_index[i]]);
   an index out of range gives ERR_BAD_INPUT for that signature.  Every key gets its cached 8-bit comb table (the last 1024 keys
   per process) and, once it has been busy enough, the 16-bit one; a key that is not a point of the curve costs ITS signatures the
   complete slow kernel, nothing else.  This form uploads keys and table addresses per call (a copy and a synchronisation):
   the _dev form is refused on a capturing stream. */
err_t bee2hip_bignVerify_keyed_batch(const bign_params *params, const octet oid_der[], size_t oid_len,
                                     const octet *hashes, const octet *sigs, const octet *pubkeys, size_t nkeys,
                                     const u32 *key_index, size_t n, err_t *codes);
err_t bee2hip_bignVerifyL_keyed_batch_dev(size_t l, const octet oid_der[], size_t oid_len,
                                          const void *d_hashes, const void *d_sigs, const octet pubkeys[], size_t nkeys,
                                          const void *d_key_index, size_t n, void *d_codes, void *stream);
/* n public keys of l/2 octets, l in {128, 192, 256}; d_pubkeys 16-byte aligned, d_codes n x err_t */
/* 8f-4 tail, device resident (private keys, one-time keys and t 4-byte aligned, hashes 16-byte).  d_codes as the
   host forms; outputs of refused items are zero.  t: n x t_len octets, or one string of t_len octets when
   t_shared != 0 (t_len <= 64 on this path; NULL = none) */
err_t bee2hip_bignPubkeyCalcL_batch_dev(size_t l, const void *d_privkeys, size_t n, void *d_pubkeys, void *d_codes,
                                        void *stream);
err_t bee2hip_bignSign2L_batch_dev(size_t l, const octet oid_der[], size_t oid_len, const void *d_hashes,
                                   const void *d_privkeys, const void *d_t, size_t t_len, int t_shared, size_t n,
                                   void *d_sigs, void *d_codes, void *stream);
err_t bee2hip_bignSignKL_batch_dev(size_t l, const octet oid_der[], size_t oid_len, const void *d_hashes,
                                   const void *d_privkeys, const void *d_ks, size_t n, void *d_sigs, void *d_codes,
                                   void *stream);
err_t bee2hip_bignPubkeyValL_batch_dev(size_t l, const void *d_pubkeys, size_t n, void *d_codes,
                                       void *stream);
err_t bee2hip_bashHash_beltMAC_batch_dev(const void *d_msgs, size_t msg_len, size_t n, size_t l,
                                         const octet key[], size_t key_len,
                                         void *d_digests, void *d_tags, void *stream);

/* Shards that already LIVE on the devices: entry i of each array belongs to device i (a pointer into its memory and an item
   count); worker i launches the single-device _dev entry on its own non-blocking stream of that device, ordered behind
   everything the device's NULL stream had been given when the call was made (a shard produced on the default stream or on a
   blocking stream needs no synchronisation; one produced on a NON-blocking stream must be complete), and the call returns when
   all are done.  Shards that share a card therefore run side by side.  Nothing is staged through the host and nothing crosses devices.  ndev = number of array entries,
   1 <= ndev <= bee2hip_device_count().  CTR: shard i holds blocks first_block + nblocks[0] + .. + nblocks[i-1] onwards of
   ONE stream with counter ctr0 (as bee2hip_beltCTR_blocks_dev); MAC / hash: d_digests or d_tags may be NULL as a whole. */
err_t bee2hip_bashF_batch_multi_dev(void *const d_states[], const size_t counts[], int ndev);
err_t bee2hip_beltCTR_blocks_multi_dev(void *const d_bufs[], const size_t nblocks[], const u32 key[8],
                                       const u32 ctr0[4], uint64_t first_block, int ndev);
err_t bee2hip_bignVerifyL_batch_multi_dev(size_t l, const octet oid_der[], size_t oid_len, const void *const d_hashes[],
                                          const void *const d_sigs[], const void *const d_pubkeys[],
                                          const size_t counts[], void *const d_codes[], int ndev);
/* one signer / a few signers, shards resident on the GPUs (the keys on the host, as in the single-device forms) */
err_t bee2hip_bignVerifyL_onekey_batch_multi_dev(size_t l, const octet oid_der[], size_t oid_len, const void *const d_hashes[],
                                                 const void *const d_sigs[], const octet pubkey[], const size_t counts[],
                                                 void *const d_codes[], int ndev);
err_t bee2hip_bignVerifyL_keyed_batch_multi_dev(size_t l, const octet oid_der[], size_t oid_len, const void *const d_hashes[],
                                                const void *const d_sigs[], const octet pubkeys[], size_t nkeys,
                                                const void *const d_key_index[], const size_t counts[], void *const d_codes[],
                                                int ndev);
err_t bee2hip_bashHash_beltMAC_batch_multi_dev(const void *const d_msgs[], size_t msg_len, const size_t counts[], size_t l,
                                               const octet key[], size_t key_len, void *const d_digests[],
                                               void *const d_tags[], int ndev);

/* ---- engine management --------------------------------------------------- */
/* bind the calling thread's engine to HIP device `device` (default: current) */
err_t bee2hip_set_device(int device);
/* block until everything queued on `stream` is done */
err_t bee2hip_sync(void *stream);
/* text of the last HIP failure on this thread ("" if none) */
const char *bee2hip_last_error(void);
/* "bee2hip <ver> gfx950" */
const char *bee2hip_version(void);
/* path of the drop-in layer's SMALL single calls (one permutation, one block, one message's serial chain, one
   signature verification): 0 = by size (default), 1 = every primitive in a kernel, 2 = the host path wherever one
   exists.  The run-time form of the environment variable BEE2HIP_FORCE=gpu|cpu; mode < 0 only queries.  Returns the
   mode that was in force.  The _dev and _multi entry points and the batch entries are never affected: they always launch
   kernels -- with ONE exception: the host-pointer bee2hip_hash_ragged hands its few longest messages (>= 64 KiB, one serial
   chain each) to host threads while the GPU takes the rest, unless the mode is 1; those messages are not uploaded, and the
   call counts once in bee2hip_path_count(0). */
int bee2hip_path_policy(int mode);
/* how many drop-in helper calls of this process went where: which = 0 host path, 1 GPU path, 2 finished on the host
   after the GPU path failed twice (a warning is printed for each of those) */
unsigned long long bee2hip_path_count(int which);
#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* BEE2HIP_H */
