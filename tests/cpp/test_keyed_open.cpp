// Registered key sets as a key cache through include/dusk_schnorr.hpp -> libdsv.so: KeySet*::verify_batch_open over
// exactly the arguments of the free verify_batch* — (signature, public key, message) triples, most under registered
// keys, some under keys the set has never seen, some tampered.  Every verdict is compared bool for bool with the
// free verify_batch* on the same objects; the miss count is what the batch was built with.  Exit code 0 = all passed.
#include <cstring>

#include "dusk_schnorr.hpp"
#include "support.hpp"

using namespace dusk_schnorr;

constexpr size_t kKeys = 7, kRegistered = 5, kItems = 240;

// Set: KeySet / KeySetDouble / KeySetVarGen; sk_of(rng) draws a secret key, pk_of(sk) its public key,
// sign(sk, rng, m) a signature, unkeyed(sigs, pks, msgs) the free verify_batch* of the scheme
template <class Set, class Key, class Secret, class SkOf, class PkOf, class Sign, class Unkeyed>
static void open(uint64_t seed, SkOf sk_of, PkOf pk_of, Sign sign, Unkeyed unkeyed) {
  using Sig = typename Set::Sig;
  Rng rng(seed);
  std::vector<Secret> sks;
  std::vector<Key> all;
  for (size_t k = 0; k < kKeys; k++) {
    sks.push_back(sk_of(rng));
    all.push_back(pk_of(sks.back()));
  }
  std::vector<Sig> sigs;
  std::vector<Key> pks;
  std::vector<BlsScalar> msgs;
  size_t unregistered = 0;
  for (size_t i = 0; i < kItems; i++) {
    const size_t k = (size_t)(rng.next() % kKeys);
    const BlsScalar m = BlsScalar::random(rng);
    sigs.push_back(sign(sks[k], rng, m));
    pks.push_back(all[k]);
    msgs.push_back(m);
    unregistered += k >= kRegistered;
  }
  // tampered under both kinds of key: every 11th item another message, one item another u
  for (size_t i = 5; i < kItems; i += 11) msgs[i] = msgs[i] + BlsScalar::one();
  sigs[20].u_ = sigs[20].u_ + JubJubScalar::from(64);
  CHECK(unregistered > 0 && unregistered < kItems);

  const std::vector<bool> want = unkeyed(sigs, pks, msgs);
  size_t yes = 0;
  for (size_t i = 0; i < kItems; i++) {
    CHECK(want[i] == !(i == 20 || (i >= 5 && (i - 5) % 11 == 0)));
    yes += want[i];
  }
  CHECK(yes > 0 && yes < kItems);

  Set keys(std::vector<Key>(all.begin(), all.begin() + kRegistered));
  CHECK(keys.size() == kRegistered);
  size_t misses = 12345;
  CHECK(keys.verify_batch_open(sigs, pks, msgs, &misses) == want);
  CHECK(misses == unregistered);
  CHECK(keys.verify_batch_open(sigs, pks, msgs) == want);
  const std::vector<uint8_t> bytes =
      keys.verify_batch_open_bytes(sigs.data(), pks.data(), msgs.data(), kItems, &misses);
  for (size_t i = 0; i < kItems; i++) CHECK(bytes[i] == (want[i] ? 1 : 0));
  CHECK(misses == unregistered);
  // an empty set: everything takes the unkeyed path; a set of all the keys: nothing does
  {
    Set none(std::vector<Key>{});
    CHECK(none.verify_batch_open(sigs, pks, msgs, &misses) == want && misses == kItems);
    Set every(all);
    CHECK(every.verify_batch_open(sigs, pks, msgs, &misses) == want && misses == 0);
  }
  // jobs: two in flight and one dropped unwaited; an empty batch
  {
    BatchJob a = keys.verify_batch_open_submit(sigs, pks, msgs), b = keys.verify_batch_open_submit(sigs, pks, msgs);
    BatchJob dropped = keys.verify_batch_open_submit(sigs, pks, msgs);
    BatchJob moved = std::move(b);
    CHECK(a.wait() == want && moved.wait() == want);
    CHECK(keys.verify_batch_open_submit(std::vector<Sig>{}, {}, {}).wait().empty());
    misses = 9;
    CHECK(keys.verify_batch_open(std::vector<Sig>{}, {}, {}, &misses).empty() && misses == 0);
  }
  // a set destroyed while its job runs: the destructor waits, the verdicts are complete
  {
    BatchJob late;
    {
      Set scoped(all);
      late = scoped.verify_batch_open_submit(sigs, pks, msgs);
    }
    CHECK(late.done());
    CHECK(late.wait() == want);
  }
  bool threw = false;
  try {
    std::vector<Key> short_pks(pks.begin(), pks.end() - 1);
    (void)keys.verify_batch_open(sigs, short_pks, msgs);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  // a key object the Rust type can hold but verify cannot use (z = 0), registered and presented: a miss, false
  {
    std::vector<Key> bad(all.begin(), all.begin() + kRegistered);
    reinterpret_cast<JubJubExtended*>(&bad[1])->z = BlsScalar::zero();
    Set with_bad(bad);
    std::vector<Key> shown = pks;
    size_t under_bad = 0;
    for (size_t i = 0; i < kItems; i++) {
      const bool is1 = std::memcmp(&pks[i], &all[1], sizeof(Key)) == 0;
      if (is1) shown[i] = bad[1], under_bad++;
    }
    CHECK(under_bad > 0);
    const std::vector<bool> got = with_bad.verify_batch_open(sigs, shown, msgs, &misses);
    CHECK(got == unkeyed(sigs, shown, msgs));
    CHECK(misses == unregistered + under_bad);
  }
}

int main() {
  open<KeySet, PublicKey, SecretKey>(
      2321, [](Rng& r) { return SecretKey::random(r); }, [](const SecretKey& sk) { return PublicKey::from(sk); },
      [](const SecretKey& sk, Rng& r, const BlsScalar& m) { return sk.sign(r, m); },
      [](const std::vector<Signature>& s, const std::vector<PublicKey>& p, const std::vector<BlsScalar>& m) {
        return verify_batch(s, p, m);
      });
  open<KeySetDouble, PublicKeyDouble, SecretKey>(
      2322, [](Rng& r) { return SecretKey::random(r); },
      [](const SecretKey& sk) { return PublicKeyDouble::from(sk); },
      [](const SecretKey& sk, Rng& r, const BlsScalar& m) { return sk.sign_double(r, m); },
      [](const std::vector<SignatureDouble>& s, const std::vector<PublicKeyDouble>& p,
         const std::vector<BlsScalar>& m) {
        return verify_batch_double(s, p, m);
      });
  open<KeySetVarGen, PublicKeyVarGen, SecretKeyVarGen>(
      2323, [](Rng& r) { return SecretKeyVarGen::random(r); },
      [](const SecretKeyVarGen& sk) { return PublicKeyVarGen::from(sk); },
      [](const SecretKeyVarGen& sk, Rng& r, const BlsScalar& m) { return sk.sign(r, m); },
      [](const std::vector<SignatureVarGen>& s, const std::vector<PublicKeyVarGen>& p,
         const std::vector<BlsScalar>& m) {
        return verify_batch_var_gen(s, p, m);
      });
  std::printf("ok: key caches of %zu of %zu keys, %zu items per scheme\n", kRegistered, kKeys, kItems);
  return 0;
}
