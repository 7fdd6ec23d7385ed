// Registered key sets through include/dusk_schnorr.hpp -> libdsv.so: the sign -> register -> verify_batch shape
// of the reference's native tests (tests/schnorr.rs, schnorr_double.rs, schnorr_var_generator.rs: sign_verify,
// test_wrong_keys) with few keys signing many messages.  Every verdict of KeySet*::verify_batch is compared
// bool for bool with the per-object `PublicKey*::verify` of the key the index names.  Exit code 0 = all passed.
#include "dusk_schnorr.hpp"
#include "support.hpp"

using namespace dusk_schnorr;

constexpr size_t kKeys = 5, kItems = 240;

// Set: KeySet / KeySetDouble / KeySetVarGen; sk_of(rng) draws a secret key, pk_of(sk) its public key,
// sign(sk, rng, m) a signature
template <class Set, class Key, class Secret, class SkOf, class PkOf, class Sign>
static void keyed(uint64_t seed, SkOf sk_of, PkOf pk_of, Sign sign) {
  using Sig = typename Set::Sig;
  Rng rng(seed);
  std::vector<Secret> sks;
  std::vector<Key> pks;
  for (size_t k = 0; k < kKeys; k++) {
    sks.push_back(sk_of(rng));
    pks.push_back(pk_of(sks.back()));
  }
  std::vector<Sig> sigs;
  std::vector<uint32_t> idx;
  std::vector<BlsScalar> msgs;
  for (size_t i = 0; i < kItems; i++) {
    const uint32_t k = (uint32_t)(rng.next() % kKeys);
    const BlsScalar m = BlsScalar::random(rng);
    sigs.push_back(sign(sks[k], rng, m));
    idx.push_back(k);
    msgs.push_back(m);
  }
  // test_wrong_keys: every 7th item is checked against another key, every 11th against another message
  std::vector<bool> want(kItems, true);
  for (size_t i = 3; i < kItems; i += 7) idx[i] = (idx[i] + 1 + (uint32_t)(i % (kKeys - 1))) % kKeys, want[i] = false;
  for (size_t i = 5; i < kItems; i += 11) msgs[i] = msgs[i] + BlsScalar::one(), want[i] = false;
  sigs[20].u_ = sigs[20].u_ + JubJubScalar::from(64), want[20] = false;

  Set keys(pks);
  CHECK(keys.size() == kKeys);
  const std::vector<uint8_t> key_ok = keys.key_ok();
  for (uint8_t b : key_ok) CHECK(b == 1);
  const std::vector<bool> ok = keys.verify_batch(sigs, idx, msgs);
  CHECK(ok.size() == kItems);
  size_t yes = 0;
  for (size_t i = 0; i < kItems; i++) {
    CHECK(ok[i] == want[i]);
    CHECK(ok[i] == pks[idx[i]].verify(sigs[i], msgs[i]));  // the per-object verify of the named key
    yes += ok[i];
  }
  CHECK(yes > 0 && yes < kItems);
  const std::vector<uint8_t> bytes = keys.verify_batch_bytes(sigs.data(), idx.data(), msgs.data(), kItems);
  for (size_t i = 0; i < kItems; i++) CHECK(bytes[i] == (ok[i] ? 1 : 0));

  // an index out of range is `false`, never a fault
  {
    std::vector<uint32_t> far = idx;
    far[0] = (uint32_t)kKeys, far[1] = 0xffffffffu;
    const std::vector<bool> got = keys.verify_batch(sigs, far, msgs);
    for (size_t i = 0; i < kItems; i++) CHECK(got[i] == (i < 2 ? false : ok[i]));
  }
  // jobs: two in flight and one dropped unwaited; a moved set keeps working, the moved-from one is empty
  {
    BatchJob a = keys.verify_batch_submit(sigs, idx, msgs), b = keys.verify_batch_submit(sigs, idx, msgs);
    BatchJob dropped = keys.verify_batch_submit(sigs, idx, msgs);
    BatchJob moved = std::move(b);
    CHECK(a.wait() == ok && moved.wait() == ok);
    CHECK(keys.verify_batch_submit(std::vector<Sig>{}, {}, {}).wait().empty());
  }
  Set other(std::move(keys));
  CHECK(other.verify_batch(sigs, idx, msgs) == ok);
  // a set destroyed while its job runs: the destructor waits, the verdicts are complete
  {
    BatchJob late;
    {
      Set scoped(pks);
      late = scoped.verify_batch_submit(sigs, idx, msgs);
    }
    CHECK(late.done());
    CHECK(late.wait() == ok);
  }
  bool threw = false;
  try {
    std::vector<uint32_t> short_idx(idx.begin(), idx.end() - 1);
    (void)other.verify_batch(sigs, short_idx, msgs);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  // a key the Rust type can hold but verify cannot use: z = 0 (from_raw_unchecked takes any coordinates)
  {
    std::vector<Key> bad = pks;
    JubJubExtended* first = reinterpret_cast<JubJubExtended*>(&bad[1]);
    first->z = BlsScalar::zero();
    Set with_bad(bad);
    const std::vector<uint8_t> kok = with_bad.key_ok();
    for (size_t k = 0; k < kKeys; k++) CHECK(kok[k] == (k == 1 ? 0 : 1));
    const std::vector<bool> got = with_bad.verify_batch(sigs, idx, msgs);
    for (size_t i = 0; i < kItems; i++) CHECK(got[i] == (idx[i] == 1 ? false : ok[i]));
  }
}

int main() {
  keyed<KeySet, PublicKey, SecretKey>(
      2321, [](Rng& r) { return SecretKey::random(r); }, [](const SecretKey& sk) { return PublicKey::from(sk); },
      [](const SecretKey& sk, Rng& r, const BlsScalar& m) { return sk.sign(r, m); });
  keyed<KeySetDouble, PublicKeyDouble, SecretKey>(
      2322, [](Rng& r) { return SecretKey::random(r); },
      [](const SecretKey& sk) { return PublicKeyDouble::from(sk); },
      [](const SecretKey& sk, Rng& r, const BlsScalar& m) { return sk.sign_double(r, m); });
  keyed<KeySetVarGen, PublicKeyVarGen, SecretKeyVarGen>(
      2323, [](Rng& r) { return SecretKeyVarGen::random(r); },
      [](const SecretKeyVarGen& sk) { return PublicKeyVarGen::from(sk); },
      [](const SecretKeyVarGen& sk, Rng& r, const BlsScalar& m) { return sk.sign(r, m); });
  std::printf("ok: key sets of %zu keys, %zu items per scheme\n", kKeys, kItems);
  return 0;
}
