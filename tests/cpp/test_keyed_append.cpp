// Key sets that grow through include/dusk_schnorr.hpp -> libdsv.so: the sign -> register -> verify_batch shape of
// tests/cpp/test_keyed.cpp (the reference's sign_verify / test_wrong_keys) with some keys registered at
// construction and the others appended afterwards.  Every verdict of KeySet*::verify_batch is compared bool for
// bool with the per-object `PublicKey*::verify` of the key the index names, before and after each append.
// Exit code 0 = all passed.
#include "dusk_schnorr.hpp"
#include "support.hpp"

using namespace dusk_schnorr;

constexpr size_t kKeys = 7, kFirst = 2, kItems = 240;

template <class Set, class Key, class Secret, class SkOf, class PkOf, class Sign>
static void grown(uint64_t seed, SkOf sk_of, PkOf pk_of, Sign sign) {
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
  for (size_t i = 3; i < kItems; i += 7) idx[i] = (idx[i] + 1 + (uint32_t)(i % (kKeys - 1))) % kKeys;
  for (size_t i = 5; i < kItems; i += 11) msgs[i] = msgs[i] + BlsScalar::one();
  std::vector<bool> want(kItems);
  size_t yes = 0;
  for (size_t i = 0; i < kItems; i++) yes += want[i] = pks[idx[i]].verify(sigs[i], msgs[i]);
  CHECK(yes > 0 && yes < kItems);

  // the verdicts of a set that holds the first k keys: an index from k on is `false`
  auto check = [&](const Set& keys, size_t k) {
    CHECK(keys.size() == k);
    for (uint8_t b : keys.key_ok()) CHECK(b == 1);
    const std::vector<bool> ok = keys.verify_batch(sigs, idx, msgs);
    for (size_t i = 0; i < kItems; i++) CHECK(ok[i] == (idx[i] < k ? want[i] : false));
  };
  const std::vector<Key> first(pks.begin(), pks.begin() + kFirst);
  Set keys(first, kKeys);
  CHECK(keys.capacity() == kKeys);
  check(keys, kFirst);
  // one key, then the rest; a batch submitted before an append is decided by the set it was submitted with or by
  // the grown one — for indices below the old k both give the same verdict
  CHECK(keys.append(std::vector<Key>(pks.begin() + kFirst, pks.begin() + kFirst + 1)) == kFirst);
  check(keys, kFirst + 1);
  BatchJob job = keys.verify_batch_submit(sigs, idx, msgs);
  CHECK(keys.append(std::vector<Key>(pks.begin() + kFirst + 1, pks.end())) == kFirst + 1);
  const std::vector<bool> during = job.wait();
  for (size_t i = 0; i < kItems; i++)
    if (idx[i] < kFirst + 1) CHECK(during[i] == want[i]);
  check(keys, kKeys);
  CHECK(keys.append({}) == kKeys);
  // full: the append throws and the set is as it was
  bool threw = false;
  try {
    (void)keys.append(first);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  check(keys, kKeys);
  // a set without reserve has no room; one that starts empty takes every key by append
  Set plain(first);
  CHECK(plain.capacity() == kFirst);
  threw = false;
  try {
    (void)plain.append(first);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  check(plain, kFirst);
  Set empty(std::vector<Key>{}, kKeys);
  check(empty, 0);
  CHECK(empty.append(pks) == 0);
  check(empty, kKeys);
  Set moved(std::move(empty));
  check(moved, kKeys);
  CHECK(empty.size() == 0 && empty.capacity() == 0);
}

int main() {
  grown<KeySet, PublicKey, SecretKey>(
      2321, [](Rng& r) { return SecretKey::random(r); }, [](const SecretKey& sk) { return PublicKey::from(sk); },
      [](const SecretKey& sk, Rng& r, const BlsScalar& m) { return sk.sign(r, m); });
  grown<KeySetDouble, PublicKeyDouble, SecretKey>(
      2322, [](Rng& r) { return SecretKey::random(r); },
      [](const SecretKey& sk) { return PublicKeyDouble::from(sk); },
      [](const SecretKey& sk, Rng& r, const BlsScalar& m) { return sk.sign_double(r, m); });
  grown<KeySetVarGen, PublicKeyVarGen, SecretKeyVarGen>(
      2323, [](Rng& r) { return SecretKeyVarGen::random(r); },
      [](const SecretKeyVarGen& sk) { return PublicKeyVarGen::from(sk); },
      [](const SecretKeyVarGen& sk, Rng& r, const BlsScalar& m) { return sk.sign(r, m); });
  std::printf("ok: key sets grown from %zu to %zu keys, %zu items per scheme\n", kFirst, kKeys, kItems);
  return 0;
}
